// tools/colour_input_to_gray.cpp — helper of tools/colour_input_ab.py: the host's scalar gray conversion (host/rvio_host.cpp to_gray, what
// System::MonoVIO ran in front of rvio_hip_frame before the device took the conversion over) on one interleaved frame, timed where it runs.
// Built by the tool with the flags of host/Makefile.
#include <chrono>
#include <cstring>

#include "../host/rvio_host.hpp"

extern "C" {
// converts `src` (w x h pixels of c interleaved bytes) as System::MonoVIO did — in place in the ImageData the input buffer handed over — and
// copies the gray image to dst; returns the seconds to_gray itself took (the ImageData is filled outside the timed span)
double colour_input_to_gray(const uint8_t* src, int w, int h, int c, int is_rgb, uint8_t* dst) {
    rvio::ImageData im;
    im.width = w; im.height = h; im.channels = c;
    im.px.assign(src, src + (size_t)w * h * c);
    const auto t0 = std::chrono::steady_clock::now();
    rvio::to_gray(&im, is_rgb != 0);
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::memcpy(dst, im.px.data(), (size_t)w * h);
    return dt;
}
}
