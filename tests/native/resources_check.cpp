// resources_check — the engine's resource handles (vortex_amd/csrc/vx_resources.hpp)
// over a fake runtime: this program defines vx_res::backend itself, over malloc
// and a log of calls, so every rule of ownership is checked on the CPU under
// ASan + UBSan (tests/test_resources_cpu.py).  It needs HIP's headers for the
// types alone and links no HIP.
//
// Prints one JSON line: {"checks": N, "failures": 0}; exit code 1 on a failure.
#include "vx_resources.hpp"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

namespace {

struct Call {
    std::string op;
    void* p;
};
std::vector<Call> g_log;
std::set<void*> g_live;     // what the fake runtime has handed out and not got back
std::set<void*> g_pinned;   // registered mappings
bool g_fail_next = false;   // the next creation fails
int g_checks = 0, g_failures = 0;

void check(bool ok, const char* what, int line) {
    ++g_checks;
    if (!ok) {
        ++g_failures;
        std::fprintf(stderr, "line %d: %s\n", line, what);
    }
}
#define CHECK(x) check((x), #x, __LINE__)

void* create(const char* op, uint64_t bytes) {
    if (g_fail_next) {
        g_fail_next = false;
        g_log.push_back({std::string(op) + " failed", nullptr});
        return nullptr;
    }
    void* p = std::malloc(bytes ? bytes : 1);
    g_live.insert(p);
    g_log.push_back({op, p});
    return p;
}
void destroy(const char* op, void* p) {
    g_log.push_back({op, p});
    if (g_live.erase(p) != 1) {  // never handed out, or given back twice
        ++g_failures;
        std::fprintf(stderr, "%s of %p, which is not alive\n", op, p);
        return;
    }
    std::free(p);
}
// the log from entry `from` on, as "op op op" (pointers checked separately)
std::string ops(size_t from) {
    std::string s;
    for (size_t k = from; k < g_log.size(); ++k) s += (k > from ? " " : "") + g_log[k].op;
    return s;
}
size_t count_op(const char* op, const void* p, size_t from = 0) {
    size_t n = 0;
    for (size_t k = from; k < g_log.size(); ++k) n += g_log[k].op == op && g_log[k].p == p;
    return n;
}

}  // namespace

namespace vx_res::backend {
void* device_alloc(uint64_t bytes) { return create("device_alloc", bytes); }
void device_free(void* p) { destroy("device_free", p); }
void* pinned_alloc(uint64_t bytes) { return create("pinned_alloc", bytes); }
void pinned_free(void* p) { destroy("pinned_free", p); }
hipEvent_t event_create(unsigned) { return static_cast<hipEvent_t>(create("event_create", 1)); }
void event_destroy(hipEvent_t e) { destroy("event_destroy", e); }
hipStream_t stream_create(unsigned, const int* priority) {
    return static_cast<hipStream_t>(create(priority ? "stream_create_priority" : "stream_create", 1));
}
void stream_synchronize(hipStream_t s) {
    g_log.push_back({"stream_synchronize", s});
    if (!g_live.count(s)) ++g_failures, std::fprintf(stderr, "synchronize of a stream that is not alive\n");
}
void stream_destroy(hipStream_t s) { destroy("stream_destroy", s); }
bool stage_register(void* p, uint64_t) {
    if (g_fail_next) {
        g_fail_next = false;
        g_log.push_back({"stage_register failed", p});
        return false;
    }
    g_pinned.insert(p);
    g_log.push_back({"stage_register", p});
    return true;
}
void stage_unregister(void* p) {
    g_log.push_back({"stage_unregister", p});
    if (g_pinned.erase(p) != 1) ++g_failures, std::fprintf(stderr, "unregister of %p, which is not registered\n", p);
}
}  // namespace vx_res::backend

namespace {

using vx_res::DeviceMem;
using vx_res::Event;
using vx_res::PinnedMem;
using vx_res::Stage;
using vx_res::Stream;

bool fill(DeviceMem& h) { return h.reserve(64); }
bool fill(PinnedMem& h) { return h.reserve(64); }
bool fill(Event& h) { return h.make(hipEventDisableTiming); }
bool fill(Stream& h) { return h.make(hipStreamNonBlocking); }
bool fill(Stage& h) { return h.make(4096, false); }

template <class H>
void* raw(const H& h) {
    return reinterpret_cast<void*>(h.get());
}

// Moves, self-move and reset of one handle type; release: the backend call that gives it back.
template <class H>
void moves(const char* release) {
    {
        H a;
        CHECK(!a && raw(a) == nullptr);
        a.reset();  // an empty handle: nothing
        CHECK(fill(a) && a);
        void* pa = raw(a);
        H b(std::move(a));  // move construction: the source is empty, nothing is released
        CHECK(!a && raw(a) == nullptr && raw(b) == pa && count_op(release, pa) == 0);
        H c;
        CHECK(fill(c));
        void* pc = raw(c);
        c = std::move(b);  // onto a non-empty target: its old resource goes, exactly once
        CHECK(!b && raw(c) == pa && count_op(release, pc) == 1 && count_op(release, pa) == 0);
        H& self = c;
        c = std::move(self);  // self-move: kept
        CHECK(c && raw(c) == pa && count_op(release, pa) == 0);
        H d;
        d = std::move(c);  // onto an empty target
        CHECK(!c && raw(d) == pa);
        d.reset();
        CHECK(!d && count_op(release, pa) == 1);
        d.reset();  // twice is harmless
        CHECK(count_op(release, pa) == 1);
        CHECK(fill(d));  // and the handle can be filled again
        void* pd = raw(d);
        g_fail_next = true;  // a failed creation leaves the handle empty
        CHECK(!fill(a) && !a);
        (void)pd;
    }  // d's resource goes with it
    CHECK(g_live.empty());
}

template <class M>
void reserves(const char* alloc, const char* release) {
    M m;
    CHECK(m.size() == 0 && m.get() == nullptr);
    CHECK(m.reserve(100) && m.size() == 100 && m.get() != nullptr);
    m.template as<uint32_t>()[24] = 7;  // the typed view is the same bytes (ASan: 100 of them)
    CHECK(m.get()[96] == 7);
    uint8_t* p = m.get();
    size_t at = g_log.size();
    CHECK(m.reserve(100) && m.reserve(40) && m.reserve(0));  // equal or smaller: nothing
    CHECK(m.get() == p && m.size() == 100 && g_log.size() == at);
    CHECK(m.reserve(101) && m.size() == 101);  // larger: free, then allocate
    CHECK(ops(at) == std::string(release) + " " + alloc && g_log[at].p == p);
    p = m.get();
    at = g_log.size();
    g_fail_next = true;  // a failing allocation: the old block is gone, the handle empty
    CHECK(!m.reserve(200) && !m && m.get() == nullptr && m.size() == 0);
    CHECK(ops(at) == std::string(release) + " " + alloc + " failed" && g_log[at].p == p);
    CHECK(m.reserve(8) && m.size() == 8 && m);  // and a later reserve works
    m.reset();
    CHECK(!m && m.size() == 0 && g_live.empty());
}

struct S {
    DeviceMem m;
    PinnedMem h;
    Event e;
    Stream s;
};

void vectors() {
    std::vector<void*> made;
    {
        std::vector<S> v;
        auto fill_from = [&](size_t from) {
            for (size_t k = from; k < v.size(); ++k) {
                CHECK(fill(v[k].m) && fill(v[k].h) && fill(v[k].e) && fill(v[k].s));
                for (void* p : {raw(v[k].m), raw(v[k].h), raw(v[k].e), raw(v[k].s)}) made.push_back(p);
            }
        };
        v.resize(3);
        fill_from(0);
        const S* before = v.data();
        v.reserve(v.capacity() + 1);  // a reallocation moves every element: nothing is released
        v.resize(v.capacity());
        CHECK(v.data() != before && g_live.size() == 12);
        fill_from(3);
        const size_t n = v.size();
        CHECK(g_live.size() == 4 * n);
        v.resize(2);  // down: the dropped elements release theirs
        CHECK(g_live.size() == 8);
        v[0] = S{};  // assignment from an empty one releases, as the engine's `s = Slot{}` did
        CHECK(g_live.size() == 4 && !v[0].m && !v[0].s);
        v.clear();
        CHECK(g_live.empty());
        v.resize(1);
        fill_from(0);
    }  // the vector's destructor
    CHECK(g_live.empty());
    for (void* p : made)  // each exactly once, whichever way it went
        CHECK(count_op("device_free", p) + count_op("pinned_free", p) + count_op("event_destroy", p) +
                  count_op("stream_destroy", p) == 1);
}

void destruction_order() {
    void *pm, *pe, *ps;
    size_t at;
    {
        struct {
            DeviceMem m;
            Event e;
            Stream s;
        } x;
        CHECK(fill(x.m) && fill(x.e) && x.s.make_with_priority(hipStreamNonBlocking, -1));
        pm = raw(x.m), pe = raw(x.e), ps = raw(x.s);
        CHECK(g_log.back().op == "stream_create_priority");
        at = g_log.size();
    }
    // the stream, declared last, is waited for and destroyed before the event and the block go
    CHECK(ops(at) == "stream_synchronize stream_destroy event_destroy device_free");
    CHECK(g_log.size() == at + 4 && g_log[at].p == ps && g_log[at + 1].p == ps && g_log[at + 2].p == pe &&
          g_log[at + 3].p == pm);
}

void stages() {
    moves<Stage>("pinned_free");
    size_t at = g_log.size();
    {
        Stage st;
        CHECK(st.make(3u << 20, true) && st && st.stage_map() == 4u << 20);  // rounded up to 2 MiB pages
        CHECK((reinterpret_cast<uintptr_t>(st.get()) & ((2u << 20) - 1)) == 0);
        st.get()[(4u << 20) - 1] = 1;  // the whole mapping is there
        CHECK(ops(at) == "stage_register" && g_log[at].p == st.get() && g_pinned.size() == 1);
        Stage moved(std::move(st));
        CHECK(!st && st.stage_map() == 0 && moved.stage_map() == 4u << 20 && g_pinned.size() == 1);
        at = g_log.size();
        g_fail_next = true;  // registration refused: the mapping goes and pinned memory stands in
        Stage fallback;
        CHECK(fallback.make(1u << 20, true) && fallback && fallback.stage_map() == 0);
        CHECK(ops(at) == "stage_register failed pinned_alloc" && g_live.size() == 1);
        at = g_log.size();
        moved = std::move(fallback);  // the mapping is unregistered (and unmapped), once
        CHECK(ops(at) == "stage_unregister" && g_pinned.empty() && moved.stage_map() == 0);
    }
    CHECK(g_live.empty() && g_pinned.empty());
}

}  // namespace

int main() {
    moves<DeviceMem>("device_free");
    moves<PinnedMem>("pinned_free");
    moves<Event>("event_destroy");
    moves<Stream>("stream_destroy");
    reserves<DeviceMem>("device_alloc", "device_free");
    reserves<PinnedMem>("pinned_alloc", "pinned_free");
    vectors();
    destruction_order();
    stages();
    CHECK(g_live.empty() && g_pinned.empty());  // (ASan's leak check backs this up)
    std::printf("{\"checks\": %d, \"failures\": %d}\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
