// Layout probe for tests/test_landmark_cov_model.py: sizeof(rvio_landmark_cov) and the offset of every member as a C++ compiler lays out the
// header's struct, one line of numbers.
#include <cstddef>
#include <cstdio>
#include "../../include/rvio_hip.h"

int main() {
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rvio_landmark_cov), offsetof(rvio_landmark_cov, feat),
                offsetof(rvio_landmark_cov, n_obs), offsetof(rvio_landmark_cov, status), offsetof(rvio_landmark_cov, reserved),
                offsetof(rvio_landmark_cov, rho), offsetof(rvio_landmark_cov, rho_sigma), offsetof(rvio_landmark_cov, p_r),
                offsetof(rvio_landmark_cov, p_w), offsetof(rvio_landmark_cov, cov_r), offsetof(rvio_landmark_cov, cov_w));
    return 0;
}
