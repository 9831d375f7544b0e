// stream_order.hpp -- how the host orders one stream against another: an owned event, a fence, and the done-mark of a stage.
// A fence ("these streams go on behind that one") is zk_streams_follow; a stage's completion is a ZkStageMark.  Host only: the
// runtime's API header and nothing of this library, so tests/stream_order_main.cpp drives it against counting stand-ins of the four
// runtime calls it makes.  Everything returns hipError_t: callers wrap the calls in ZK_HIP as they do the runtime's own.
#pragma once
#include <hip/hip_runtime_api.h>

// One hipEvent_t, owned: created by the first record() with the flags given at construction, destroyed with the object.
// Move-only; a moved-from object is empty.
class ZkEvent {
    hipEvent_t e = nullptr;
    unsigned flags;
    void reset() {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }

   public:
    explicit ZkEvent(unsigned flags_ = hipEventDisableTiming) : flags(flags_) {}
    ZkEvent(ZkEvent&& o) noexcept : e(o.e), flags(o.flags) { o.e = nullptr; }
    ZkEvent& operator=(ZkEvent&& o) noexcept {
        if (this != &o) {
            reset();
            e = o.e;
            flags = o.flags;
            o.e = nullptr;
        }
        return *this;
    }
    ZkEvent(const ZkEvent&) = delete;
    ZkEvent& operator=(const ZkEvent&) = delete;
    ~ZkEvent() { reset(); }
    hipError_t record(hipStream_t st) {
        if (!e) {
            const hipError_t r = hipEventCreateWithFlags(&e, flags);
            if (r != hipSuccess) {
                e = nullptr;
                return r;
            }
        }
        return hipEventRecord(e, st);
    }
    hipEvent_t get() const { return e; }
    explicit operator bool() const { return e != nullptr; }
};

// The `count` streams of `waiters` go on behind what `from` carries now: one event, recorded on `from`, one wait per waiter, in
// order.  The first failing call's error comes back and no later waiter is touched; the event goes on every path.
inline hipError_t zk_streams_follow(hipStream_t from, const hipStream_t* waiters, int count) {
    if (count <= 0) return hipSuccess;
    ZkEvent e;
    hipError_t r = e.record(from);
    for (int k = 0; k < count && r == hipSuccess; k++) r = hipStreamWaitEvent(waiters[k], e.get(), 0);
    return r;
}

// Where a stage of a job was completed: set(st) records `done` behind the stage's last launch on st, order(st) puts st behind it.
// A consumer on the stream the mark was set on is ordered by the stream itself and an unset mark orders nothing: neither makes a
// runtime call (a wait is 3.9 us of host time).
struct ZkStageMark {
    ZkEvent done;
    hipStream_t stream = nullptr;
    hipError_t set(hipStream_t st) {
        stream = st;
        return done.record(st);
    }
    hipError_t order(hipStream_t st) const {
        if (!done || st == stream) return hipSuccess;
        return hipStreamWaitEvent(st, done.get(), 0);
    }
};
