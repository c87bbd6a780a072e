// Layout probe for tests/test_window_pose_abi.py: sizeof(rvio_window_pose) and the offset of every member as a C++ compiler lays out the
// header's struct, one line of numbers.
#include <cstddef>
#include <cstdio>
#include "../../include/rvio_hip.h"

int main() {
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rvio_window_pose), offsetof(rvio_window_pose, seq), offsetof(rvio_window_pose, img_count),
                offsetof(rvio_window_pose, age), offsetof(rvio_window_pose, n_clones), offsetof(rvio_window_pose, reserved), offsetof(rvio_window_pose, p),
                offsetof(rvio_window_pose, q), offsetof(rvio_window_pose, pose_cov));
    return 0;
}
