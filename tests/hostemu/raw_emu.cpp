// raw_emu.cpp — r-vio_amd/csrc/raw.h (the per-pixel arithmetic of raw16_kernel / raw16_kernel4 / bayer_kernel / bayer_kernel4) compiled with g++ and
// walked the way the kernel forms walk an image: sample by sample, four pixels at a time through the dwords that hold them, and — for the mosaics —
// one pixel from nine clamped loads (plain form) or a 64-lane segment whose lanes own four pixels and take the sample left and right of their group
// from the neighbouring lane (wide form).  tests/test_raw_arith.py compares each walk against NumPy.
#include "../../r-vio_amd/csrc/raw.h"

extern "C" {
void raw_emu_depth(const uint16_t* v, long n, uint8_t* dst) {
    for (long i = 0; i < n; ++i) dst[i] = (uint8_t)raw_depth8(v[i]);
}
// plain form: n pixels of ch 16-bit samples each -> n gray bytes
void raw_emu_px16(const uint16_t* src, long n, int ch, int bgr, uint8_t* dst) {
    const GrayW w = gray_weights(bgr);
    for (long i = 0; i < n; ++i) dst[i] = (uint8_t)(ch == 1 ? raw_depth8(src[i]) : raw16_px(src[i * ch], src[i * ch + 1], src[i * ch + 2], w));
}
// wide form: n pixels (a multiple of 4) as n / 4 groups of 2 ch dwords -> n / 4 dwords of four gray bytes
int raw_emu_wide16(const uint32_t* src, long n, int ch, int bgr, uint32_t* dst) {
    if (n % 4 != 0 || (ch != 1 && ch != 3 && ch != 4)) return -1;
    const GrayW w = gray_weights(bgr);
    for (long g = 0; g < n / 4; ++g)
        dst[g] = ch == 1 ? raw16_4<1>(src + 2 * g, w) : ch == 3 ? raw16_4<3>(src + 6 * g, w) : raw16_4<4>(src + 8 * g, w);
    return 0;
}
// plain mosaic form: every output from bayer_at.  bits: 8 | 16; stride in samples
int raw_emu_bayer(const void* img, int bits, long stride, int w, int h, int pat, uint8_t* dst) {
    if (w < 3 || h < 3 || pat < 0 || pat > 3) return -1;
    const BayerP b = bayer_pattern(pat);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            dst[(size_t)y * w + x] = (uint8_t)(bits == 16 ? bayer_at<uint16_t>((const uint16_t*)img, stride, w, h, x, y, b)
                                                          : bayer_at<uint8_t>((const uint8_t*)img, stride, w, h, x, y, b));
    return 0;
}
static uint32_t sample(const void* img, int bits, long stride, int x, int y) {
    return bits == 16 ? ((const uint16_t*)img)[(size_t)y * stride + x] : ((const uint8_t*)img)[(size_t)y * stride + x];
}
// wide mosaic form: segments of 256 pixels, 64 lanes of four; a lane past the row's end holds the row's last group again, lane 0 / lane 63 take the
// sample outside the segment from a clamped address, every other lane from its neighbour's group
int raw_emu_bayer_wide(const void* img, int bits, long stride, int w, int h, int pat, uint8_t* dst) {
    if (w < 4 || w % 4 != 0 || h < 3 || pat < 0 || pat > 3) return -1;
    const BayerP b = bayer_pattern(pat);
    for (int y = 0; y < h; ++y) {
        const int yc = raw_clampi(y, 1, h - 2);
        for (int x0 = 0; x0 < w; x0 += 256) {
            uint32_t grp[64][3][4];
            for (int lane = 0; lane < 64; ++lane) {
                const int g = x0 / 4 + lane < w / 4 - 1 ? x0 / 4 + lane : w / 4 - 1;
                for (int r = 0; r < 3; ++r) for (int k = 0; k < 4; ++k) grp[lane][r][k] = sample(img, bits, stride, 4 * g + k, yc - 1 + r);
            }
            for (int lane = 0; lane < 64; ++lane) {
                if (x0 + 4 * lane >= w) continue;
                const int xh = lane < 32 ? (x0 - 1 > 0 ? x0 - 1 : 0) : (x0 + 256 < w - 1 ? x0 + 256 : w - 1);
                uint32_t s[3][6];
                for (int r = 0; r < 3; ++r) {
                    const uint32_t e = sample(img, bits, stride, xh, yc - 1 + r);
                    for (int k = 0; k < 4; ++k) s[r][k + 1] = grp[lane][r][k];
                    s[r][0] = lane == 0 ? e : grp[lane - 1][r][3];
                    s[r][5] = lane == 63 ? e : grp[lane + 1][r][0];
                }
                const uint32_t o = bayer4(s, x0 + 4 * lane, yc, w, b, bits == 16);
                for (int k = 0; k < 4; ++k) dst[(size_t)y * w + x0 + 4 * lane + k] = (uint8_t)(o >> (8 * k));
            }
        }
    }
    return 0;
}
}
