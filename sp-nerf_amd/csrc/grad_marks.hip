// The backward's side stream, the gradient-readiness marks and their spnerf_grad_mark* entries.
#include <atomic>
#include <mutex>

#include "grad_marks.h"
#include "mlp_layout.h"
#include "mlp_options.h"

namespace spn {

// backward: 2 = weight gradients on a second stream beside the dX chain; 1 = one stream (default:
// measured on MI355X, the two streams' GEMMs contend for HBM / L2 and the step got 3% slower,
// in eager mode and as a captured graph alike — C4 at 512 rays 4.99 -> 5.15 ms)
int g_bwd_streams = 1;

static Side g_side[64];

Side* side_stream() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    Side& sd = g_side[dev];
    if (!sd.ok) {
        if (hipStreamCreateWithFlags(&sd.s, hipStreamNonBlocking) != hipSuccess) return nullptr;
        for (auto& e : sd.ev)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        sd.ok = true;
    }
    return &sd;
}

int32_t stream_dep(Side* sd, hipStream_t from, hipStream_t to) {
    if (!sd || from == to) return SPNERF_OK;
    hipEvent_t e = sd->ev[sd->next];
    sd->next = (sd->next + 1) % 64;
    SPN_HIP(hipEventRecord(e, from));
    SPN_HIP(hipStreamWaitEvent(to, e, 0));
    return SPNERF_OK;
}

// Gradient readiness marks (spnerf_grad_marks): when armed, a backward records mark k's event
// on the stream that finishes that group of weight gradients — mark 0 after the output heads',
// 1 + (L-1-i) after trunk layer i's, L+1 at the end (per-ray parameters) — so that a data-parallel
// caller can all-reduce each group while the rest of the backward runs.  One event set per device.
// Inside a HIP-graph capture the marks are the graph's own dependency edges: the all-reduces must
// then be captured into the same graph (dp.GradBuckets).
int g_marks_flags = hipEventDisableTiming;  // option "grad_marks_flags": hipEventCreateWithFlags flags (before the first arm)
namespace {
struct Marks {
    hipEvent_t ev[64] = {};
    std::atomic<bool> ok{false};
    std::atomic<uint64_t> recorded{0};   // bit k: mark k recorded at least once since the events were made
};
Marks g_marks[64];
std::mutex g_marks_mu;                   // creation only (a watchdog thread may query concurrently)
int g_marks_armed = 0;

// The mark events of device `dev`, created on first use when `create` (on that device: the
// calling thread's current device is the caller's, e.g. the rank's own GPU); nullptr when they do
// not exist and `create` is false — a query from another thread never creates them.
Marks* marks_of(int dev, bool create) {
    if (dev < 0 || dev >= 64) return nullptr;
    Marks& m = g_marks[dev];
    if (m.ok.load(std::memory_order_acquire)) return &m;
    if (!create) return nullptr;
    std::lock_guard<std::mutex> lock(g_marks_mu);
    if (!m.ok.load(std::memory_order_relaxed)) {
        for (auto& e : m.ev)
            if (hipEventCreateWithFlags(&e, (unsigned)g_marks_flags) != hipSuccess) return nullptr;
        m.ok.store(true, std::memory_order_release);
    }
    return &m;
}

Marks* marks_of_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    return marks_of(dev, true);
}
}  // namespace

int32_t grad_mark(int k, hipStream_t s) {
    if (!g_marks_armed) return SPNERF_OK;
    Marks* m = marks_of_device();
    SPN_ARG(m && k >= 0 && k < 64, "grad_mark: no mark events");
    // a plain record: under stream capture it becomes a dependency edge of the graph being
    // captured (a wait on it from another stream of the same capture joins that stream to the
    // graph); this HIP runtime refuses external event-record nodes (hipEventRecordExternal)
    SPN_HIP(hipEventRecord(m->ev[k], s));
    m->recorded.fetch_or(uint64_t(1) << k, std::memory_order_relaxed);
    return SPNERF_OK;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_grad_marks(const spnerf_model_cfg* cfg, int32_t* mark_of_param, int32_t n_params) {
    Dims d;
    SPN_TRY(make_dims(cfg, &d));
    PIdx x;
    auto specs = param_specs(d, &x);
    SPN_ARG(mark_of_param && n_params == (int32_t)specs.size(), "spnerf_grad_marks: need one slot per parameter");
    SPN_ARG(d.L + 2 <= 64, "spnerf_grad_marks: too many layers");
    const int end = d.L + 1;
    for (size_t i = 0; i < specs.size(); ++i) mark_of_param[i] = 0;  // output heads (mark 0)
    for (int i = 0; i < d.L; ++i) {
        const int m = 1 + (d.L - 1 - i);
        mark_of_param[x.fcb[i]] = m;
        // the semantic columns of layer 0 / the skip layer come from per-ray sums at the end
        mark_of_param[x.fcW[i]] = (d.sem && (i == 0 || i == d.skip)) ? end : m;
    }
    // per-ray parameters and columns (step 7 of the backward)
    for (int pi : {x.emb, x.s1W, x.k1W, x.k1b, x.k2W, x.k2b, x.b1W})
        if (pi >= 0) mark_of_param[pi] = end;
    return d.L + 2;
}

extern "C" int32_t spnerf_grad_marks_arm(int32_t on) {
    if (on) SPN_ARG(marks_of_device() != nullptr, "spnerf_grad_marks_arm: cannot create the mark events");
    g_marks_armed = on ? 1 : 0;
    return SPNERF_OK;
}

extern "C" int32_t spnerf_grad_mark_wait(int32_t mark, void* stream) {
    Marks* m = marks_of_device();
    SPN_ARG(m && mark >= 0 && mark < 64, "spnerf_grad_mark_wait: bad mark");
    SPN_HIP(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), m->ev[mark], 0));
    return SPNERF_OK;
}

extern "C" int32_t spnerf_grad_mark_query(int32_t device, int32_t mark) {
    SPN_ARG(device >= 0 && device < 64 && mark >= 0 && mark < 64, "spnerf_grad_mark_query: bad device or mark");
    Marks* m = marks_of(device, false);
    if (!m || !(m->recorded.load(std::memory_order_relaxed) & (uint64_t(1) << mark))) return 2;   // never recorded
    int cur = -1;
    SPN_HIP(hipGetDevice(&cur));
    if (cur != device) SPN_HIP(hipSetDevice(device));
    const hipError_t e = hipEventQuery(m->ev[mark]);
    if (cur != device) SPN_HIP(hipSetDevice(cur));
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) return 0;
    SPN_HIP(e);
    return 0;
}
