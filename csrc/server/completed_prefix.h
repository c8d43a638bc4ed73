// Completed prefix of a stream's pending FIFO (Shard::completion_loop).
//
// Task i of the FIFO is either real (it holds a slot whose event was recorded
// on the stream) or a null-slot task (a submit failure queued only to carry
// its done callback). Events of real tasks fire in FIFO order. The completed
// prefix ends at the first real task whose event has not fired; a null-slot
// task is complete exactly when every real task before it is, so it never
// lets a task in front of it be taken early.
//
// Host-only and free of HIP includes, so the search is tested on its own
// (tests/test_completed_prefix.py).
#pragma once

#include <cstddef>

namespace ifs {

// has_slot(i): is task i real?  fired(i): has real task i's event fired? (the
// expensive question: one hipEventQuery). Returns how many tasks at the front
// of the n pending may be taken: the index of the first real task whose event
// has not fired, or n.
//
// Binary search: fired(i) is asked at most ceil(log2(n + 1)) times. A null
// task at the probe point is stepped over towards the front, to the nearest
// real task of the open range, which costs no query; a queue without null
// tasks is probed at exactly (lo + hi) / 2 each time.
template <typename HasSlot, typename Fired>
size_t completed_prefix(size_t n, HasSlot&& has_slot, Fired&& fired) {
    // Invariant: every real task in [0, lo) has fired; hi is n or a real task
    // that had not fired when asked. The answer is hi once the range is empty.
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        size_t r = mid;
        while (r > lo && !has_slot(r)) r--;
        if (!has_slot(r)) {
            lo = mid + 1;  // [lo, mid] holds null tasks only: nothing to ask
            continue;
        }
        if (fired(r))
            lo = mid + 1;  // (r, mid] are null tasks
        else
            hi = r;
    }
    return hi;
}

}  // namespace ifs
