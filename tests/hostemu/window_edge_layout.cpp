// Layout probe for tests/test_window_graph_abi.py: sizeof(rvio_window_edge) and the offset of every member as a C++ compiler lays out the
// header's struct, one line of numbers.
#include <cstddef>
#include <cstdio>
#include "../../include/rvio_hip.h"

int main() {
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rvio_window_edge), offsetof(rvio_window_edge, seq),
                offsetof(rvio_window_edge, img_count_new), offsetof(rvio_window_edge, img_count_old), offsetof(rvio_window_edge, age_new),
                offsetof(rvio_window_edge, age_old), offsetof(rvio_window_edge, n_clones), offsetof(rvio_window_edge, reserved),
                offsetof(rvio_window_edge, p), offsetof(rvio_window_edge, q), offsetof(rvio_window_edge, cov));
    return 0;
}
