// The owned event, the fence and the stage mark of zk-mpc_amd/csrc/stream_order.hpp against stand-ins of the four runtime calls they
// make: a self-checking driver for tests/test_stream_order_host.py.  No HIP library is linked: the stand-ins below count live events,
// log every call with its stream, and fail the k-th call on request.  Prints "ok" and returns 0, or names the first expectation that
// failed.
#include "stream_order.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>

struct Call {
    char what;              // 'c'reate, 'd'estroy, 'r'ecord, 'w'ait
    hipStream_t stream;     // record / wait
    hipEvent_t event;
    unsigned flags;         // create
    bool operator==(const Call& o) const { return what == o.what && stream == o.stream && event == o.event && flags == o.flags; }
};
static std::vector<Call> calls;
static std::set<hipEvent_t> live;
static int destroyed_twice = 0;
static long fail_at = -1;       // the index in `calls` of the call that fails (it is logged, and does nothing)
static char event_ids[64];      // addresses only: an event is never dereferenced
static size_t next_event = 0;
static const hipError_t FAILS[4] = {hipErrorOutOfMemory, hipErrorInvalidValue, hipErrorInvalidHandle, hipErrorNotReady};

static bool failing(const Call& c) {
    calls.push_back(c);
    return (long)calls.size() - 1 == fail_at;
}
extern "C" hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned flags) {
    if (failing({'c', nullptr, nullptr, flags})) return FAILS[0];
    *event = (hipEvent_t)&event_ids[next_event++ % sizeof event_ids];
    calls.back().event = *event;
    live.insert(*event);
    return hipSuccess;
}
extern "C" hipError_t hipEventDestroy(hipEvent_t event) {
    calls.push_back({'d', nullptr, event, 0});
    if (!live.erase(event)) destroyed_twice++;
    return hipSuccess;
}
extern "C" hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
    return failing({'r', stream, event, 0}) ? FAILS[1] : hipSuccess;
}
extern "C" hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned flags) {
    return failing({'w', stream, event, flags}) ? FAILS[2] : hipSuccess;
}

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); }  \
    } while (0)

static char stream_ids[8];
static hipStream_t S(int k) { return (hipStream_t)&stream_ids[k]; }
static void fresh(long fail = -1) {
    CHECK(live.empty() && destroyed_twice == 0);
    calls.clear();
    fail_at = fail;
}
static size_t count(char what) {
    size_t n = 0;
    for (const Call& c : calls) n += c.what == what;
    return n;
}

static_assert(!std::is_copy_constructible<ZkEvent>::value && !std::is_copy_assignable<ZkEvent>::value, "ZkEvent copies");
static_assert(std::is_move_constructible<ZkEvent>::value && std::is_move_assignable<ZkEvent>::value, "ZkEvent does not move");
static_assert(!std::is_copy_constructible<ZkStageMark>::value, "ZkStageMark copies");

struct ThreeMarks { ZkStageMark a, b, c; int tag = 0; };      // the shape of a job: what a growing vector moves

int main() {
    // ---- zk_streams_follow ----
    const hipStream_t w3[3] = {S(1), S(2), S(3)};
    fresh();
    CHECK(zk_streams_follow(S(0), w3, 0) == hipSuccess && zk_streams_follow(S(0), nullptr, -1) == hipSuccess && calls.empty());
    for (int n : {1, 3}) {
        fresh();
        CHECK(zk_streams_follow(S(0), w3, n) == hipSuccess);
        CHECK(calls.size() == (size_t)n + 3 && live.empty());
        const hipEvent_t e = calls[0].event;
        CHECK((calls[0] == Call{'c', nullptr, e, hipEventDisableTiming}) && (calls[1] == Call{'r', S(0), e, 0}));
        for (int k = 0; k < n; k++) CHECK((calls[2 + k] == Call{'w', w3[k], e, 0}));
        CHECK((calls[2 + n] == Call{'d', nullptr, e, 0}));
    }
    for (long f = 0; f < 5; f++) {      // the create, the record, each of the three waits
        fresh(f);
        CHECK(zk_streams_follow(S(0), w3, 3) == FAILS[f == 0 ? 0 : f == 1 ? 1 : 2]);
        CHECK(live.empty() && destroyed_twice == 0);
        CHECK(count('c') == 1 && count('r') == (f >= 1 ? 1u : 0u) && count('w') == (f >= 2 ? (size_t)f - 1 : 0u));      // nothing behind the failing call
        CHECK(count('d') == (f >= 1 ? 1u : 0u));                                                                       // (a failed create left nothing to destroy)
        for (long k = 2; k <= f; k++) CHECK(calls[(size_t)k].stream == w3[k - 2]);
    }

    // ---- ZkEvent ----
    fresh();
    {
        ZkEvent a;
        CHECK(!a && a.get() == nullptr && calls.empty());       // nothing before the first record
        CHECK(a.record(S(0)) == hipSuccess && a.record(S(1)) == hipSuccess);
        CHECK(count('c') == 1 && count('r') == 2 && a && a.get() == calls[0].event && calls[0].flags == hipEventDisableTiming);
        CHECK(calls[1].stream == S(0) && calls[2].stream == S(1) && calls[2].event == a.get());
        const hipEvent_t ea = a.get();
        ZkEvent b(std::move(a));                                 // move construction: the source is empty, nothing is destroyed yet
        CHECK(!a && b && b.get() == ea && count('d') == 0 && live.size() == 1);
        ZkEvent c(0);                                            // flags 0: an event that keeps time
        CHECK(c.record(S(2)) == hipSuccess && calls.back().event == c.get() && live.size() == 2);
        const hipEvent_t ec = c.get();
        CHECK(calls[calls.size() - 2].what == 'c' && calls[calls.size() - 2].flags == 0);
        c = std::move(b);                                        // move assignment onto a live event: the old one goes first
        CHECK((calls.back() == Call{'d', nullptr, ec, 0}) && c.get() == ea && !b && live.size() == 1 && *live.begin() == ea);
        ZkEvent& self = c;
        c = std::move(self);                                     // (onto itself: nothing happens)
        CHECK(c.get() == ea && live.size() == 1);
        CHECK(a.record(S(3)) == hipSuccess && a.get() != ea && live.size() == 2);      // a moved-from object is an empty one: usable again
    }
    CHECK(live.empty() && destroyed_twice == 0 && count('d') == 3 && count('c') == 3);
    fresh(0);
    {
        ZkEvent a;
        CHECK(a.record(S(0)) == FAILS[0] && !a && calls.size() == 1);                  // a failed create: no record, still empty
        CHECK(a.record(S(0)) == hipSuccess && a);                                       // ... and the next record tries again
    }
    CHECK(live.empty() && destroyed_twice == 0);

    // ---- ZkStageMark ----
    fresh();
    {
        ZkStageMark m;
        CHECK(m.order(S(1)) == hipSuccess && m.order(nullptr) == hipSuccess && calls.empty());      // unset: no call at all
        CHECK(m.set(S(1)) == hipSuccess && m.stream == S(1) && calls.size() == 2 && (calls[1] == Call{'r', S(1), m.done.get(), 0}));
        CHECK(m.order(S(1)) == hipSuccess && calls.size() == 2);                                    // its own stream: no call
        CHECK(m.order(S(2)) == hipSuccess && calls.size() == 3 && (calls[2] == Call{'w', S(2), m.done.get(), 0}));
        const ZkStageMark& cm = m;                                                                   // (a consumer holds the job const)
        CHECK(cm.order(S(3)) == hipSuccess && calls.size() == 4 && calls[3].stream == S(3));
        CHECK(m.set(S(2)) == hipSuccess && m.stream == S(2) && count('c') == 1 && live.size() == 1);      // set twice: one live event
        CHECK(m.order(S(2)) == hipSuccess && calls.size() == 5);
        CHECK(m.order(S(1)) == hipSuccess && calls.size() == 6 && (calls[5] == Call{'w', S(1), m.done.get(), 0}));
    }
    CHECK(live.empty() && destroyed_twice == 0);
    fresh(2);
    {
        ZkStageMark m;
        CHECK(m.set(S(1)) == hipSuccess && m.order(S(2)) == FAILS[2]);                              // a failing wait comes back
    }
    CHECK(live.empty() && destroyed_twice == 0);
    fresh();
    {
        std::vector<ThreeMarks> v;
        for (int k = 0; k < 9; k++) {                            // grows from nothing: every mark moves several times
            v.emplace_back();
            v.back().tag = k;
            CHECK(v.back().a.set(S(1)) == hipSuccess && v.back().c.set(S(2)) == hipSuccess);        // (b stays unset)
        }
        CHECK(live.size() == 18 && count('d') == 0 && destroyed_twice == 0);
        for (int k = 0; k < 9; k++) CHECK(v[(size_t)k].tag == k && v[(size_t)k].a.done && !v[(size_t)k].b.done && v[(size_t)k].c.stream == S(2));
        std::vector<ThreeMarks> u(std::move(v));
        CHECK(live.size() == 18 && u[4].a.order(S(1)) == hipSuccess && count('w') == 0);
    }
    CHECK(live.empty() && destroyed_twice == 0 && count('d') == 18);
    printf("ok\n");
    return 0;
}
