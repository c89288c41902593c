// The backward's side stream and the gradient-readiness marks (grad_marks.hip).
#pragma once
#include "common.h"

namespace spn {
#pragma GCC visibility push(hidden)  // internal to the library

// The backward's second stream: the weight-gradient GEMMs, their slab reductions and the per-ray
// parameter sums run there, beside the dX chain on the caller's stream, joined by events
// (fork: main → side after an input is produced; join: side → main at the end, so the caller
// sees the usual stream order).  Inside a captured HIP graph the same calls record a fork/join
// graph.  One library-owned non-blocking stream and an event ring per device.
struct Side {
    hipStream_t s = nullptr;
    hipEvent_t ev[64] = {};
    int next = 0;
    bool ok = false;
};
Side* side_stream();  // of the current device; nullptr when it cannot be made
// `to` waits for everything issued so far on `from` (no-op without a side stream)
int32_t stream_dep(Side* sd, hipStream_t from, hipStream_t to);

// records mark k on s when the marks are armed (spnerf_grad_marks_arm)
int32_t grad_mark(int k, hipStream_t s);

#pragma GCC visibility pop
}  // namespace spn
