// Host build of csrc/ring_span.h for tests/test_ring_span.py: the read window of the handle's record rings as plain C functions.
// With -DRING_SPAN_MAIN the same file is a stand-alone program that walks the test's sweep and checks every span against the formula's own
// invariants (exit status 0: clean) — the form in which the header is run under -fsanitize=address,undefined.
#include "../../r-vio_amd/csrc/ring_span.h"

extern "C" {
// out: first seq served, count, start slot, length of the first span
void rs_span(long long newest, long long cap, long long first_seq, long long max_n, long long* out) {
    const RingSpan s = ring_span(newest, cap, first_seq, max_n);
    out[0] = s.first; out[1] = s.count; out[2] = s.slot0; out[3] = s.n0;
}
long long rs_slot(long long seq, long long cap) { return ring_slot(seq, cap); }
long long rs_index(long long seq, long long cap, int batch, int instance) { return (long long)ring_index(seq, cap, batch, instance); }
}

#ifdef RING_SPAN_MAIN
#include <cstdio>
#include <vector>
int main() {
    long long spans = 0, bad = 0;
    for (long long cap = 1; cap <= 5; ++cap)
        for (long long newest = 0; newest <= 3 * cap + 1; ++newest) {
            // the ring as the device leaves it: slot s holds the seq written there last (0: never written)
            std::vector<long long> ring((size_t)cap, 0);
            for (long long seq = 1; seq <= newest; ++seq) ring[(size_t)ring_slot(seq, cap)] = seq;
            for (long long first = -2; first <= newest + 2; ++first)
                for (long long max_n = 0; max_n <= cap + 2; ++max_n) {
                    const RingSpan s = ring_span(newest, cap, first, max_n);
                    ++spans;
                    if (s.count < 0 || s.count > max_n || s.count > cap || s.n0 < 0 || s.n0 > s.count) { ++bad; continue; }
                    for (long long j = 0; j < s.count; ++j) {   // read as the getter copies: first span from slot0, second from slot 0
                        const long long slot = j < s.n0 ? s.slot0 + j : j - s.n0;
                        if (slot < 0 || slot >= cap || ring[(size_t)slot] != s.first + j) ++bad;
                    }
                }
        }
    std::printf("ring_span: %lld spans, %lld bad\n", spans, bad);
    return bad ? 1 : 0;
}
#endif
