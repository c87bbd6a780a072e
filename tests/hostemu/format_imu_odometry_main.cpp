// Reads rvio_imu_pose records (raw, 104 bytes each) from the file named on the command line and prints each through the host's own
// format_imu_odometry (host/rvio_host.cpp): tests/test_imu_odometry_abi.py parses the lines back and compares all 11 columns bit for bit.
#include <cstdio>
#include <vector>
#include "rvio_host.hpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    rvio_imu_pose r;
    while (std::fread(&r, sizeof r, 1, f) == 1) std::fputs(rvio::format_imu_odometry(r).c_str(), stdout);
    std::fclose(f);
    return 0;
}
