// ring_span.h — the layout and the read window of the handle's record rings (odometry, IMU-rate odometry), host arithmetic only: plain C++17,
// no HIP, so that tests/hostemu/ring_span_emu.cpp compiles it with g++ (tests/test_ring_span.py sweeps it against a list model of the ring).
//
// Layout: records carry a 1-based sequence number; record `seq` of instance i of a ring of `cap` records per instance lies at
//   ring[((seq - 1) % cap) * batch + i]
// — the records of one seq are contiguous over the instances (one launch writes them), those of one instance lie `batch` records apart.
#pragma once
#include <algorithm>
#include <cstddef>

// the slot of record seq (>= 1) in a ring of cap (>= 1) records per instance, and its first record's index
inline long long ring_slot(long long seq, long long cap) { return (seq - 1) % cap; }
inline size_t ring_index(long long seq, long long cap, int batch, int instance = 0) { return (size_t)ring_slot(seq, cap) * (size_t)batch + (size_t)instance; }

// What a read of at most max_n records from first_seq on is served: the records first .. first + count - 1, oldest first — n0 of them from
// slot0 on, the other count - n0 from slot 0 on (the range wraps around the end of the ring at most once).
struct RingSpan { long long first, count, slot0, n0; };
// newest: the seq of the last record written (0: none yet).  The ring still holds newest - cap + 1 .. newest; nothing before seq 1 exists.
inline RingSpan ring_span(long long newest, long long cap, long long first_seq, long long max_n) {
    const long long lo = std::max<long long>(std::max<long long>(first_seq, newest - cap + 1), 1);
    const long long cnt = std::max<long long>(0, std::min<long long>(newest - lo + 1, max_n));
    if (cnt == 0) return RingSpan{lo, 0, 0, 0};
    const long long s0 = ring_slot(lo, cap);
    return RingSpan{lo, cnt, s0, std::min(cnt, cap - s0)};
}
