// gray_emu.cpp — r-vio_amd/csrc/gray.h (the per-pixel arithmetic of gray_kernel / gray_kernel4) compiled with g++ and walked over a pixel
// list the way the two kernel forms walk a row: byte by byte, and four pixels at a time through the dwords that hold them.
// tests/test_gray_arith.py feeds it all 2^24 (R, G, B) triples.
#include "../../r-vio_amd/csrc/gray.h"

extern "C" {
// byte form: n pixels of ch bytes each -> n gray bytes
void gray_emu_bytes(const uint8_t* src, long n, int ch, int bgr, uint8_t* dst) {
    const GrayW w = gray_weights(bgr);
    for (long i = 0; i < n; ++i) dst[i] = (uint8_t)gray_px(src[i * ch], src[i * ch + 1], src[i * ch + 2], w);
}
// wide form: n pixels (a multiple of 4) as n / 4 groups of ch dwords -> n / 4 dwords of four gray bytes
int gray_emu_wide(const uint32_t* src, long n, int ch, int bgr, uint32_t* dst) {
    if (n % 4 != 0 || (ch != 3 && ch != 4)) return -1;
    const GrayW w = gray_weights(bgr);
    for (long g = 0; g < n / 4; ++g) dst[g] = ch == 3 ? gray4<3>(src + 3 * g, w) : gray4<4>(src + 4 * g, w);
    return 0;
}
}
