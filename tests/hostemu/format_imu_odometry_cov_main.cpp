// Reads rvio_imu_pose records (raw, 104 bytes each) from the first file and the paired rvio_imu_cov records (raw, 376 bytes each) from the
// second, and prints each pair through the host's own format_imu_odometry_cov (host/rvio_host.cpp): tests/test_imu_cov_abi.py parses the lines
// back and compares all 38 columns bit for bit.
#include <cstdio>
#include "rvio_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    std::FILE* g = std::fopen(argv[2], "rb");
    if (!f || !g) return 3;
    rvio_imu_pose r;
    rvio_imu_cov c;
    while (std::fread(&r, sizeof r, 1, f) == 1 && std::fread(&c, sizeof c, 1, g) == 1) std::fputs(rvio::format_imu_odometry_cov(r, c).c_str(), stdout);
    std::fclose(f);
    std::fclose(g);
    return 0;
}
