// block_rounds_check.cpp — CPU harness for the round driver of the v2 and hybrid
// files calls (vx_block_rounds.hpp), used by tests/test_block_rounds_cpu.py under
// ASan + UBSan.  Not the product; no GPU.
//
// argv: dir.  The program writes a torrent's files there (byte p of file f is
// pattern(f, p)) and drives vx_block_rounds::run with the real reader pool, the
// real vx_merkle::Rounds (once with a hole predicate) and the real
// vx_hybrid::Rounds over a fake device:
//  * one posix_memalign'd stage per slot;
//  * enqueue checks every read of the round against the pattern (so the driver
//    waited for the ticket), keeps a copy of the stage's [0, round.bytes) and
//    marks the slot busy with a countdown `lag`;
//  * a non-blocking done-query is one tick for all busy slots, and a slot whose
//    countdown has run out completes; a blocking one completes its slot at once;
//    lag < 0: only a blocking query completes;
//  * on completion the stage is compared with the copy: a read that landed while
//    the "copy" was in flight shows up as a difference;
//  * a stage requested for a busy slot is an error.
// stdout: a JSON line with the runs made and the mismatches and errors found;
// every error is named on stderr.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "vx_block_rounds.hpp"
#include "vx_hybrid_rounds.hpp"

static uint8_t pattern(size_t f, uint64_t p) { return (uint8_t)(p * 131 + f * 17 + (p >> 8) + (p >> 16)); }

static uint64_t g_errors = 0, g_mismatches = 0;
static std::string g_case;
static void error(const std::string& what) {
    ++g_errors;
    std::fprintf(stderr, "%s: %s\n", g_case.c_str(), what.c_str());
}

constexpr int kInjected = -77;
enum class Fail { None, Stage, Enqueue, Done };

template <class Round>
struct Fake {
    const size_t nslots;
    const int lag;
    const uint64_t stage_bytes;
    const std::vector<Round>& want;  // the planner's rounds, in its order
    Fail fail = Fail::None;
    size_t fail_round = 0;  // the round whose stage request, enqueue or done-query fails
    std::vector<uint8_t*> stages;
    std::vector<std::vector<uint8_t>> copy;
    std::vector<uint8_t> busy;
    std::vector<int> left;
    size_t staged = 0, enqueued = 0, completed = 0, max_outstanding = 0, enqueued_at_failure = 0;
    const vx_files::Readers* rd = nullptr;
    uint64_t read_upto = 0;  // the bytes of the reads of the rounds enqueued: all of them have been read

    Fake(size_t n, int lag_, uint64_t bytes, const std::vector<Round>& rounds)
        : nslots(n), lag(lag_), stage_bytes(bytes), want(rounds), stages(n, nullptr), copy(n), busy(n, 0), left(n, 0) {
        for (auto& s : stages) {
            void* raw = nullptr;
            if (posix_memalign(&raw, 4096, (size_t)stage_bytes)) std::abort();
            s = static_cast<uint8_t*>(raw);
        }
    }
    ~Fake() {
        for (uint8_t* s : stages) std::free(s);
    }
    int injected() {
        enqueued_at_failure = enqueued;
        return kInjected;
    }
    void complete(size_t si) {
        if (std::memcmp(stages[si], copy[si].data(), copy[si].size()) != 0) {
            ++g_mismatches;
            error("slot " + std::to_string(si) + ": the stage changed while its copy was in flight");
        }
        busy[si] = 0;
        ++completed;
    }
    void drain() {  // what the caller's stream syncs do after run()
        for (size_t si = 0; si < nslots; ++si)
            if (busy[si]) complete(si);
    }
    int done(size_t si, bool block) {
        if (fail == Fail::Done && staged == fail_round) return injected();
        if (block) {
            if (busy[si]) complete(si);
            return 0;
        }
        for (size_t s = 0; s < nslots; ++s) {
            if (!busy[s] || lag < 0) continue;
            if (left[s] == 0)
                complete(s);
            else
                --left[s];
        }
        return busy[si] ? vx_block_rounds::kNotYet : 0;
    }
    uint8_t* stage(size_t si, int* rc) {
        *rc = 0;
        if (fail == Fail::Stage && staged == fail_round) {
            *rc = injected();
            return nullptr;
        }
        if (si != staged % nslots) error("round " + std::to_string(staged) + " read into slot " + std::to_string(si));
        if (busy[si]) error("a stage was requested for busy slot " + std::to_string(si));
        ++staged;
        max_outstanding = std::max(max_outstanding, staged - completed);
        return stages[si];
    }
    int enqueue(size_t si, const Round& r) {
        if (fail == Fail::Enqueue && enqueued == fail_round) return injected();
        const size_t k = enqueued++;
        if (si != k % nslots) error("round " + std::to_string(k) + " enqueued on slot " + std::to_string(si));
        if (busy[si]) error("round " + std::to_string(k) + " enqueued on a busy slot");
        for (const auto& x : r.reads) read_upto += x.len;
        if (rd->bytes_read() < read_upto) error("round " + std::to_string(k) + " enqueued before its reads were done");
        if (k >= want.size() || r.bytes != want[k].bytes || r.file_bytes != want[k].file_bytes ||
            r.reads.size() != want[k].reads.size()) {
            error("round " + std::to_string(k) + " is not the planner's round " + std::to_string(k));
            return 0;
        }
        for (size_t j = 0; j < r.reads.size(); ++j) {
            const auto &x = r.reads[j], &w = want[k].reads[j];
            if (x.file != w.file || x.file_off != w.file_off || x.len != w.len || stage_offset(x) != stage_offset(w))
                error("round " + std::to_string(k) + ": read " + std::to_string(j) + " differs from the planner's");
            if (stage_offset(x) + x.len > stage_bytes) {
                error("round " + std::to_string(k) + ": a read passes the stage");
                continue;
            }
            for (uint64_t at = 0; at < x.len; ++at)
                if (stages[si][stage_offset(x) + at] != pattern(x.file, x.file_off + at)) {
                    ++g_mismatches;
                    error("round " + std::to_string(k) + ": read " + std::to_string(j) + " is not in the stage");
                    break;
                }
        }
        copy[si].assign(stages[si], stages[si] + r.bytes);
        busy[si] = 1;
        left[si] = lag;
        return 0;
    }
};

struct Torrent {
    std::vector<uint64_t> lens;
    std::vector<int> fds;
    uint32_t pl;
    uint64_t n_pieces;
};

// One run of the driver over `make()`'s planner; fail != None: the injected
// failure and how many rounds must have been enqueued before it.
template <class Round, class Planner>
static void drive(const Torrent& t, const std::function<Planner()>& make, size_t nslots, int lag, uint64_t stage_bytes,
                  Fail fail = Fail::None, size_t fail_round = 0, size_t want_before = 0) {
    std::vector<Round> want;
    {
        Planner p = make();
        Round r;
        while (p.next(r)) want.push_back(r);
    }
    uint64_t want_file = 0, want_copy = 0, read_bytes = 0;
    std::vector<uint8_t> bad(t.n_pieces ? t.n_pieces : 1, 0);
    const std::vector<vx_files::FileSpan> none;
    Fake<Round> dev(nslots, lag, stage_bytes, want);
    dev.fail = fail;
    dev.fail_round = fail_round;
    vx_files::Readers rd(4, none, t.fds, t.pl, bad.data(), 0, nullptr, true);
    dev.rd = &rd;
    Planner plan = make();
    vx_block_rounds::Totals totals;
    const int rc = vx_block_rounds::run<Round>(
        plan, rd, nslots, dev, [&dev](size_t si, const Round& r) { return dev.enqueue(si, r); }, totals);
    // no read is outstanding: every read of every round that got a stage has been counted
    for (size_t k = 0; k < dev.staged && k < want.size(); ++k)
        for (const auto& x : want[k].reads) read_bytes += x.len;
    if (rd.bytes_read() != read_bytes) error("reads were outstanding when the driver returned");
    const size_t at_return = dev.enqueued;
    dev.drain();
    for (size_t k = 0; k < dev.enqueued && k < want.size(); ++k) {
        want_file += want[k].file_bytes;
        want_copy += want[k].bytes;
    }
    if (totals.rounds != dev.enqueued || totals.file_bytes != want_file || totals.copy_bytes != want_copy)
        error("the totals are not the sums over the rounds enqueued");
    if (dev.max_outstanding > nslots) error("more than nslots rounds between read-submitted and completed");
    for (uint8_t b : bad)
        if (b) error("a piece was marked bad");
    if (fail == Fail::None) {
        if (rc != 0) error("the driver returned " + std::to_string(rc));
        if (dev.enqueued != want.size()) error("not every round of the planner was enqueued");
        return;
    }
    if (rc != kInjected) error("the driver returned " + std::to_string(rc) + ", not the injected code");
    if (dev.enqueued_at_failure != want_before)
        error(std::to_string(dev.enqueued_at_failure) + " rounds were enqueued before the failure, not " +
              std::to_string(want_before));
    if (at_return != dev.enqueued_at_failure) error("a round was enqueued after the failure");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    Torrent t;
    t.pl = 65536;
    t.lens = {0,     1,      16384,  16385,  65536,  65537,  299999, 123457, 200000,
              77777, 262144, 31000,  288888, 250001, 180224, 299008, 270000, 222222};
    t.fds.assign(t.lens.size(), -1);
    for (size_t f = 0; f < t.lens.size(); ++f) {
        const std::string path = dir + "/f" + std::to_string(f);
        std::vector<uint8_t> body((size_t)t.lens[f]);
        for (size_t p = 0; p < body.size(); ++p) body[p] = pattern(f, p);
        FILE* out = std::fopen(path.c_str(), "wb");
        if (!out || (!body.empty() && std::fwrite(body.data(), 1, body.size(), out) != body.size())) return 3;
        std::fclose(out);
        t.fds[f] = open(path.c_str(), O_RDONLY | O_CLOEXEC);
    }
    t.n_pieces = vx_merkle::torrent_pieces(t.lens.data(), t.lens.size(), t.pl);
    const uint32_t kb = vx_merkle::kBlock;
    // every fifth block of the odd files is a hole: not read, not in the stage
    const vx_merkle::HolePredicate holes = [](uint32_t f, uint64_t off, uint32_t) {
        return f % 2 == 1 && off / vx_merkle::kBlock % 5 == 3;
    };
    auto merkle = [&](uint32_t bpr, uint64_t count, vx_merkle::HolePredicate hole) {
        return std::function<vx_merkle::Rounds()>([&t, bpr, count, hole] {
            return vx_merkle::Rounds(t.lens.data(), t.lens.size(), t.pl, 0, count, bpr,
                                     vx_merkle::Rounds::window_for(bpr, t.pl), 2 * bpr + t.pl / vx_merkle::kBlock, 4,
                                     hole);
        });
    };
    auto hybrid = [&](uint64_t stage) {
        return std::function<vx_hybrid::Rounds()>([&t, stage] {
            return vx_hybrid::Rounds(t.lens.data(), t.lens.size(), t.pl, t.n_pieces, 0, t.n_pieces, stage,
                                     vx_hybrid::chunk_for(t.pl, stage));
        });
    };
    uint64_t sweeps = 0, failures = 0;
    const int lags[] = {0, 1, 7, -1};
    for (uint32_t bpr : {4u, 16u})
        for (size_t nslots : {1, 2, 3, 5})
            for (int lag : lags) {
                const std::string at = " blocks " + std::to_string(bpr) + " slots " + std::to_string(nslots) + " lag " +
                                       std::to_string(lag);
                g_case = "v2" + at;
                drive<vx_merkle::Round>(t, merkle(bpr, t.n_pieces, nullptr), nslots, lag, (uint64_t)bpr * kb);
                g_case = "hybrid" + at;
                drive<vx_hybrid::Round>(t, hybrid((uint64_t)bpr * kb), nslots, lag, (uint64_t)bpr * kb);
                sweeps += 2;
            }
    g_case = "v2 with holes";
    drive<vx_merkle::Round>(t, merkle(16, t.n_pieces, holes), 3, 1, 16 * kb);
    g_case = "a planner without a round";
    drive<vx_merkle::Round>(t, merkle(16, 0, nullptr), 3, 1, 16 * kb);
    sweeps += 2;

    // Failures at the first, a middle and the last round, with a device that is
    // done at the first query (lag 0) and one that never is before a blocking
    // query (lag -1).  How many rounds are enqueued before the failing call
    // follows from the ring's rules, depth = nslots - 1:
    //  * enqueue of round k: k;
    //  * stage request of round k: it follows round k's read-ahead.  lag 0: the
    //    read runs depth rounds ahead, max(0, k - depth).  lag -1: a round past
    //    the first nslots is read only when it is next to be enqueued, k (the
    //    first nslots: 0);
    //  * done-query for round k's slot (k >= nslots; the "first" is k = nslots):
    //    the first query.  lag 0: when the read-ahead reaches k, k - depth.
    //    lag -1: right behind round k - 1's read, k - 1 (k = nslots: at
    //    k - depth, behind the first nslots reads); one slot: k.
    auto fail_all = [&](const std::string& name, auto make, uint64_t stage_bytes, auto round_tag) {
        using Round = decltype(round_tag);
        size_t n = 0;
        {
            auto p = make();
            Round r;
            while (p.next(r)) ++n;
        }
        for (size_t nslots : {1, 3})
            for (int lag : {0, -1}) {
                const size_t depth = nslots - 1;
                for (size_t k : {(size_t)0, n / 2, n - 1}) {
                    g_case = name + " slots " + std::to_string(nslots) + " lag " + std::to_string(lag) + " round " +
                             std::to_string(k);
                    drive<Round>(t, make, nslots, lag, stage_bytes, Fail::Enqueue, k, k);
                    const size_t before_stage = lag == 0 ? (k > depth ? k - depth : 0) : (k < nslots ? 0 : k);
                    drive<Round>(t, make, nslots, lag, stage_bytes, Fail::Stage, k, before_stage);
                    const size_t q = std::max(k, nslots);  // the first round that has a done-query
                    const size_t before_done = depth == 0 ? q : (lag == 0 || q == nslots) ? q - depth : q - 1;
                    drive<Round>(t, make, nslots, lag, stage_bytes, Fail::Done, q, before_done);
                    failures += 3;
                }
            }
    };
    fail_all("v2 failure", merkle(16, t.n_pieces, nullptr), 16 * kb, vx_merkle::Round{});
    fail_all("hybrid failure", hybrid(16 * kb), 16 * kb, vx_hybrid::Round{});

    for (int fd : t.fds)
        if (fd >= 0) close(fd);
    std::printf("{\"sweeps\": %llu, \"failures\": %llu, \"mismatches\": %llu, \"errors\": %llu}\n",
                (unsigned long long)sweeps, (unsigned long long)failures, (unsigned long long)g_mismatches,
                (unsigned long long)g_errors);
    return g_errors ? 1 : 0;
}
