// raw.h — the gray conversion of raw sensor data: what cv_bridge::toCvShare(msg, MONO8) does in front of Tracker::track (rvio_mono.cc:64) for the
// encodings a machine-vision camera publishes besides mono8 and 8-bit colour.  cv_bridge converts COLOUR first, at the source's bit depth, and
// DEPTH second, so every 16-bit format is "gray at 16 bits, then 16 -> 8".
//
//   depth     convertTo(CV_8U, 255. / 65535.): round-to-nearest of v / 257 (no tie: 257 k + 128.5 is no integer) = (v + 128) / 257 <= 255
//   colour16  y16 = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14 in unsigned 32 bits (the weights sum to 1 << 14: <= 65535), then the depth step
//   Bayer     cvtColor COLOR_Bayer*2GRAY, bilinear, with kR = 4899, kG = 9617, kB = 1868, for an interior pixel (1 <= x <= W - 2, 1 <= y <= H - 2)
//               red / blue site, own colour C, opposite D:   Y = (4 kC p + kG (N + S + E + W) + kD (NE + NW + SE + SW) + 32768) >> 16
//               green site, horizontal neighbours Ch, vertical Cv:   Y = (2 kG p + kCh (E + W) + kCv (N + S) + 16384) >> 15
//             column 0 copies column 1 and column W - 1 column W - 2, then row 0 copies row 1 and row H - 1 row H - 2: output (x, y) is the interior
//             formula AT (clamp(x, 1, W - 2), clamp(y, 1, H - 2)) — the whole 3 x 3 window moves, and so does the parity that names the site.
//             16-bit worst case 65535 * 65536 + 32768 < 2^32.  A 16-bit mosaic takes the same formulas, then the depth step.
// Patterns are named as ROS does, by the top-left 2 x 2 block in reading order: RGGB is (0,0) = R, (1,0) = G, (0,1) = G, (1,1) = B.  The colour of a
// site follows from the ABSOLUTE parity of (x, y).
//
// The per-pixel code of raw16_kernel / raw16_kernel4 / bayer_kernel / bayer_kernel4 (raw.hip) lives here so that g++ compiles the very same text
// (tests/hostemu/raw_emu.cpp, tests/test_raw_arith.py).
#pragma once
#include <stddef.h>
#include "gray.h"

GRAY_FN uint32_t raw_depth8(uint32_t v) { return (v + 128u) / 257u; }

// one 16-bit pixel whose first three samples are c0 c1 c2 in memory order
GRAY_FN uint32_t raw16_px(uint32_t c0, uint32_t c1, uint32_t c2, GrayW w) { return raw_depth8(gray_px(c0, c1, c2, w)); }

// sample i of a run of 16-bit samples held in dwords (little endian)
GRAY_FN uint32_t raw_half(const uint32_t* v, int i) { return (v[i >> 1] >> (16 * (i & 1))) & 65535u; }

// four adjacent 16-bit pixels of CH samples each as the 2 CH dwords that hold them -> four gray bytes in one dword
template <int CH>
GRAY_FN uint32_t raw16_4(const uint32_t* v, GrayW w) {
    uint32_t out = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k)
        out |= (CH == 1 ? raw_depth8(raw_half(v, k)) : raw16_px(raw_half(v, CH * k), raw_half(v, CH * k + 1), raw_half(v, CH * k + 2), w)) << (8 * k);
    return out;
}

// A Bayer pattern is where its red site lies in the 2 x 2 block (blue lies diagonally opposite): the low two bits of the format's value
//   0 RGGB (0,0)   1 BGGR (1,1)   2 GBRG (0,1)   3 GRBG (1,0)
struct BayerP { int rx, ry; };
GRAY_FN BayerP bayer_pattern(int p) { BayerP b; b.rx = (p == 1 || p == 3) ? 1 : 0; b.ry = (p == 1 || p == 2) ? 1 : 0; return b; }

// the interior formula at the site (x, y): p its sample, hs = E + W, vs = N + S, ds = NE + NW + SE + SW; at the source's depth (8 or 16 bits)
GRAY_FN uint32_t bayer_px(uint32_t p, uint32_t hs, uint32_t vs, uint32_t ds, int x, int y, BayerP b) {
    const int px = (x ^ b.rx) & 1, py = (y ^ b.ry) & 1;   // (0,0): red site, (1,1): blue site, (1,0): green in a red row, (0,1): green in a blue row
    if (px == py) {
        const uint32_t kc = px ? GRAY_B2Y : GRAY_R2Y, kd = px ? GRAY_R2Y : GRAY_B2Y;
        return (4u * kc * p + GRAY_G2Y * (hs + vs) + kd * ds + 32768u) >> 16;
    }
    const uint32_t kh = py ? GRAY_B2Y : GRAY_R2Y, kv = py ? GRAY_R2Y : GRAY_B2Y;
    return (2u * GRAY_G2Y * p + kh * hs + kv * vs + 16384u) >> 15;
}

GRAY_FN int raw_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// One output pixel straight from the mosaic (the plain kernel form, and the host): T = uint8_t | uint16_t, row stride in SAMPLES.  Every address is
// inside the image for any (x, y) inside it, W >= 3, H >= 3.
template <typename T>
GRAY_FN uint32_t bayer_at(const T* img, size_t stride, int w, int h, int x, int y, BayerP b) {
    const int xc = raw_clampi(x, 1, w - 2), yc = raw_clampi(y, 1, h - 2);
    const T* r0 = img + (size_t)(yc - 1) * stride + (xc - 1);
    const T* r1 = r0 + stride;
    const T* r2 = r1 + stride;
    const uint32_t a0 = r0[0], a1 = r0[1], a2 = r0[2], b0 = r1[0], b1 = r1[1], b2 = r1[2], c0 = r2[0], c1 = r2[1], c2 = r2[2];
    const uint32_t y0 = bayer_px(b1, b0 + b2, a1 + c1, a0 + a2 + c0 + c2, xc, yc, b);
    return sizeof(T) == 2 ? raw_depth8(y0) : y0;
}

// Four adjacent outputs x4 .. x4 + 3 (x4 % 4 == 0, w % 4 == 0) of the row whose window rows are s[0..2] (already the rows yc - 1, yc, yc + 1 of the
// clamped row yc): s[r][0] is the sample left of the group, s[r][1..4] the group, s[r][5] the sample right of it.  The samples outside the image
// (left of column 0, right of column w - 1) may hold anything: the outputs that would use them are the two border columns, which copy their neighbour.
//
// The same values as bayer_px, arranged for a wave: a row holds ONE of red / blue (its colour C, the other being D) at the columns of one parity and
// green at the others, so kC, kD and that parity are the same for every lane of a row and, with x4 % 4 == 0, the site kind of each of the four outputs
// is fixed once the parity is known — one formula per output, no per-lane choice.  C0: the parity of the columns that hold C.
template <int C0>
GRAY_FN void bayer4_row(const uint32_t s[3][6], uint32_t kc, uint32_t kd, uint32_t* o) {
    uint32_t vs[6];   // N + S of every column of the window
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int j = 0; j < 6; ++j) vs[j] = s[0][j] + s[2][j];
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const uint32_t p = s[1][k + 1], hs = s[1][k] + s[1][k + 2];
        if ((k & 1) == C0) o[k] = (4u * kc * p + GRAY_G2Y * (hs + vs[k + 1]) + kd * (vs[k] + vs[k + 2]) + 32768u) >> 16;
        else o[k] = (2u * GRAY_G2Y * p + kc * hs + kd * vs[k + 1] + 16384u) >> 15;
    }
}
GRAY_FN uint32_t bayer4(const uint32_t s[3][6], int x4, int yc, int w, BayerP b, bool wide16) {
    const bool red_row = ((yc ^ b.ry) & 1) == 0;
    const uint32_t kc = red_row ? GRAY_R2Y : GRAY_B2Y, kd = red_row ? GRAY_B2Y : GRAY_R2Y;
    uint32_t o[4];
    if (((red_row ? b.rx : b.rx ^ 1) & 1) == 0) bayer4_row<0>(s, kc, kd, o);
    else bayer4_row<1>(s, kc, kd, o);
    if (wide16) {
#ifdef __HIPCC__
#pragma unroll
#endif
        for (int k = 0; k < 4; ++k) o[k] = raw_depth8(o[k]);
    }
    if (x4 == 0) o[0] = o[1];
    if (x4 + 4 == w) o[3] = o[2];
    return o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
}
