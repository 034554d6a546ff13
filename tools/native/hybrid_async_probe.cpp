// hybrid_async_probe.cpp — the download path of a hybrid (v1 + v2) torrent two
// ways, side by side: one process, one context, the same registered buffers
// (one mmap per buffer, as vortex's BufferPool has, buf_pool.rs:92-98), legs
// alternating so all see the same machine state.
//
//   leg A  vx_hybrid_submit: one submit per piece, pads implied.
//   leg B  the way before it: vx_submit (over the caller's padded copy where a
//          piece has a pad) plus vx_merkle_submit; a piece is complete when
//          both completions have arrived.  The v1 submits of a batch go first,
//          then its v2 submits (alternating them would launch a slot per piece),
//          and the padded copies are made once, outside the timed legs: both
//          in leg B's favour.
//   leg V  vx_merkle_submit alone, for scale.
//
//   burst  every buffer submitted once as fast as the submits take them, then
//          flushed and polled dry: GiB/s of the pieces' data bytes per leg.
//   loop   the event loop's shape: `batch` pieces submitted, one vx_flush,
//          then polls until all are back; per piece the time from its (first)
//          submit to the poll that completed it: p50 / p99 per leg.
//
// Every pad_every-th piece ends a file: 3/4 of a piece and 5 bytes of data, the
// rest pad.  Every verdict is checked (expected rows come from the bulk calls
// first; every 97th piece's rows are planted wrong).  Prints one JSON line.
//
// usage: hybrid_async_probe burst <piece_len> [total_bytes=2147483648] [reps=5] [pad_every=16]
//        hybrid_async_probe loop  <piece_len> [batch=32] [batches=200] [reps=5] [pad_every=16]
#include <sys/mman.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "vx_hash.h"

using clk = std::chrono::steady_clock;

static double since(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }

static double pct(std::vector<double> v, double p) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[std::min(v.size() - 1, (size_t)(p * (double)(v.size() - 1) + 0.5))];
}

static std::string list(const std::vector<double>& v, double scale) {
    std::string s = "[";
    char b[32];
    for (size_t i = 0; i < v.size(); ++i) {
        std::snprintf(b, sizeof b, "%s%.3f", i ? ", " : "", v[i] * scale);
        s += b;
    }
    return s + "]";
}

enum Leg { kHybrid = 0, kPair = 1, kMerkle = 2, kLegs = 3 };
static const char* kLegName[kLegs] = {"A", "B", "V"};

struct Probe {
    vx_ctx* ctx = nullptr;
    uint32_t plen = 0, log2w = 0, nbuf = 0;
    std::vector<uint8_t*> bufs, padded;  // padded[b]: data || zeros, registered too (NULL: the piece has no pad)
    std::vector<uint32_t> lens, pads;
    std::vector<uint8_t> sha1, roots;    // expected rows, every 97th wrong
    std::vector<clk::time_point> t_sub;
    std::vector<uint8_t> arrived;
    std::vector<vx_completion> cq1{4096};
    std::vector<vx_merkle_completion> cq2{4096};
    std::vector<vx_hybrid_completion> cq3{4096};
    uint64_t wrong = 0;

    int submit_all(Leg leg) {
        for (uint32_t b = 0; b < nbuf; ++b) {
            t_sub[b] = clk::now();
            arrived[b] = 0;
            int rc = 0;
            if (leg == kHybrid)
                rc = vx_hybrid_submit(ctx, b, bufs[b], lens[b], pads[b], log2w, &sha1[(size_t)b * 20],
                                      &roots[(size_t)b * 32]);
            else if (leg == kPair)
                rc = vx_submit(ctx, b, pads[b] ? padded[b] : bufs[b], lens[b] + pads[b], &sha1[(size_t)b * 20]);
            else
                rc = vx_merkle_submit(ctx, b, bufs[b], lens[b], log2w, &roots[(size_t)b * 32]);
            if (rc) return rc;
        }
        if (leg == kPair)
            for (uint32_t b = 0; b < nbuf; ++b)
                if (int rc = vx_merkle_submit(ctx, b, bufs[b], lens[b], log2w, &roots[(size_t)b * 32])) return rc;
        return 0;
    }
    void complete(uint32_t b, clk::time_point now, std::vector<double>* lat) {
        if (lat) lat->push_back(since(t_sub[b], now));
    }
    // One round of polls; returns how many pieces became complete.
    int64_t poll(Leg leg, std::vector<double>* lat) {
        int64_t complete_n = 0;
        if (leg == kHybrid) {
            const int64_t k = vx_hybrid_poll(ctx, cq3.data(), cq3.size());
            if (k < 0) return k;
            const auto now = clk::now();
            for (int64_t j = 0; j < k; ++j) {
                const uint32_t b = (uint32_t)cq3[j].tag;
                wrong += cq3[j].matched != (b % 97 ? 3 : 0);
                complete(b, now, lat);
            }
            return k;
        }
        if (leg == kPair) {
            const int64_t k = vx_poll(ctx, cq1.data(), cq1.size());
            if (k < 0) return k;
            const auto now = clk::now();
            for (int64_t j = 0; j < k; ++j) {
                const uint32_t b = (uint32_t)cq1[j].tag;
                wrong += (cq1[j].matched != 0) != (b % 97 != 0);
                if (++arrived[b] == 2) complete(b, now, lat), ++complete_n;
            }
        }
        const int64_t k = vx_merkle_poll(ctx, cq2.data(), cq2.size());
        if (k < 0) return k;
        const auto now = clk::now();
        for (int64_t j = 0; j < k; ++j) {
            const uint32_t b = (uint32_t)cq2[j].tag;
            wrong += (cq2[j].matched != 0) != (b % 97 != 0);
            if (++arrived[b] == (leg == kPair ? 2 : 1)) complete(b, now, lat), ++complete_n;
        }
        return complete_n;
    }
};

int main(int argc, char** argv) {
    if (argc < 3 || (std::strcmp(argv[1], "burst") && std::strcmp(argv[1], "loop"))) {
        std::fprintf(stderr,
                     "usage: %s burst piece_len [total_bytes] [reps] [pad_every]\n"
                     "       %s loop piece_len [batch] [batches] [reps] [pad_every]\n",
                     argv[0], argv[0]);
        return 2;
    }
    const bool burst = !std::strcmp(argv[1], "burst");
    Probe p;
    p.plen = (uint32_t)std::strtoul(argv[2], nullptr, 0);
    const uint64_t total = burst && argc > 3 ? std::strtoull(argv[3], nullptr, 0) : 2ull << 30;
    const uint32_t batch = !burst && argc > 3 ? (uint32_t)std::atoi(argv[3]) : 32;
    const uint32_t batches = !burst && argc > 4 ? (uint32_t)std::atoi(argv[4]) : 200;
    const int reps = std::max(1, argc > (burst ? 4 : 5) ? std::atoi(argv[burst ? 4 : 5]) : 5);
    const uint32_t pad_every = argc > (burst ? 5 : 6) ? (uint32_t)std::atoi(argv[burst ? 5 : 6]) : 16;
    if (p.plen < VX_MERKLE_BLOCK || (p.plen & (p.plen - 1)) || batch == 0 || batches == 0) {
        std::fprintf(stderr, "piece_len must be a power of two >= 16384; batch and batches > 0\n");
        return 2;
    }
    while (((uint32_t)VX_MERKLE_BLOCK << p.log2w) < p.plen) ++p.log2w;
    p.nbuf = burst ? (uint32_t)std::max<uint64_t>(1, total / p.plen) : batch;
    vx_config cfg;
    vx_config_default(&cfg, p.plen);
    if (int rc = vx_create(&cfg, &p.ctx)) {
        std::fprintf(stderr, "vx_create: %d %s\n", rc, vx_last_error());
        return 1;
    }
    std::mt19937_64 rng(p.plen ^ 0xB47);
    p.bufs.resize(p.nbuf);
    p.padded.assign(p.nbuf, nullptr);
    p.lens.assign(p.nbuf, p.plen);
    p.pads.assign(p.nbuf, 0);
    p.t_sub.resize(p.nbuf);
    p.arrived.assign(p.nbuf, 0);
    auto pinned = [&](uint8_t** out) {
        void* m = mmap(nullptr, p.plen, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_POPULATE, -1, 0);
        if (m == MAP_FAILED) return 1;
        *out = static_cast<uint8_t*>(m);
        if (int rc = vx_register_host_buffer(p.ctx, m, p.plen)) {
            std::fprintf(stderr, "register: %d %s\n", rc, vx_last_error());
            return 1;
        }
        return 0;
    };
    std::vector<const uint8_t*> v1_ptrs(p.nbuf), v2_ptrs(p.nbuf);
    std::vector<uint32_t> v1_lens(p.nbuf, p.plen);
    uint64_t data_bytes = 0;
    uint32_t n_padded = 0;
    for (uint32_t b = 0; b < p.nbuf; ++b) {
        if (pinned(&p.bufs[b])) return 1;
        for (size_t i = 0; i < p.plen / 8; ++i) reinterpret_cast<uint64_t*>(p.bufs[b])[i] = rng();
        if (pad_every && b % pad_every == 1) {  // this piece ends a file
            p.lens[b] = p.plen / 4 * 3 + 5;
            p.pads[b] = p.plen - p.lens[b];
            if (pinned(&p.padded[b])) return 1;
            std::memcpy(p.padded[b], p.bufs[b], p.lens[b]);  // (the mmap's rest is zero already)
            ++n_padded;
        }
        v1_ptrs[b] = p.pads[b] ? p.padded[b] : p.bufs[b];
        v2_ptrs[b] = p.bufs[b];
        data_bytes += p.lens[b];
    }
    // the expected rows, from the bulk calls (tested against hashlib elsewhere)
    p.sha1.resize((size_t)p.nbuf * 20);
    p.roots.resize((size_t)p.nbuf * 32);
    std::vector<uint8_t> zeros((size_t)p.nbuf * 32), verdicts(p.nbuf);
    int rc = vx_sha1_batch(p.ctx, v1_ptrs.data(), v1_lens.data(), p.nbuf, p.sha1.data());
    if (!rc)
        rc = vx_merkle_verify_batch(p.ctx, v2_ptrs.data(), p.lens.data(), nullptr, p.nbuf, p.plen, zeros.data(),
                                    verdicts.data(), p.roots.data());
    if (rc) {
        std::fprintf(stderr, "expected rows: %d %s\n", rc, vx_last_error());
        return 1;
    }
    for (uint32_t b = 0; b < p.nbuf; b += 97) {
        p.sha1[(size_t)b * 20 + 3] ^= 1;
        p.roots[(size_t)b * 32 + 3] ^= 1;
    }

    // One leg: `rounds` times submit every buffer, flush, poll until all are complete.
    auto leg = [&](Leg which, uint32_t rounds, std::vector<double>* lat, double* seconds) -> int {
        const auto t0 = clk::now();
        for (uint32_t r = 0; r < rounds; ++r) {
            if (int e = p.submit_all(which)) return e;
            if (int e = vx_flush(p.ctx)) return e;
            for (uint64_t got = 0; got < p.nbuf;) {
                const int64_t k = p.poll(which, lat);
                if (k < 0) return (int)k;
                got += (uint64_t)k;
                if (since(t0, clk::now()) > 120) return VX_EBUSY;  // never in practice: a stuck batch
            }
        }
        *seconds = since(t0, clk::now());
        return 0;
    };
    const uint32_t rounds = burst ? 1 : batches;
    std::vector<double> fig[kLegs], p99[kLegs];  // per leg: GiB/s (burst) or p50 seconds (loop)
    double s = 0;
    for (int k = 0; k < kLegs && !rc; ++k) rc = leg((Leg)k, burst ? 1 : 8, nullptr, &s);  // warm every kind's buffers
    for (int r = 0; r < reps && !rc; ++r) {
        for (int k = 0; k < kLegs && !rc; ++k) {
            std::vector<double> lat;
            rc = leg((Leg)k, rounds, &lat, &s);
            if (burst) {
                fig[k].push_back((double)data_bytes / s / (double)(1ull << 30));
            } else {
                fig[k].push_back(pct(lat, 0.5));
                p99[k].push_back(pct(lat, 0.99));
            }
        }
    }
    if (rc) {
        std::fprintf(stderr, "leg failed: %d %s\n", rc, vx_last_error());
        return 1;
    }
    vx_stats st{};
    vx_get_stats(p.ctx, &st);
    for (uint32_t b = 0; b < p.nbuf; ++b) {
        vx_unregister_host_buffer(p.ctx, p.bufs[b]);
        munmap(p.bufs[b], p.plen);
        if (p.padded[b]) {
            vx_unregister_host_buffer(p.ctx, p.padded[b]);
            munmap(p.padded[b], p.plen);
        }
    }
    vx_destroy(p.ctx);
    const double scale = burst ? 1.0 : 1e3;
    std::printf("{\"mode\": \"%s\", \"piece_len\": %u, \"pieces\": %u, \"padded_pieces\": %u, \"data_bytes\": %llu, "
                "\"batches_per_leg\": %u, \"reps\": %d, \"unit\": \"%s\"",
                burst ? "burst" : "loop", p.plen, p.nbuf, n_padded, (unsigned long long)data_bytes, rounds, reps,
                burst ? "GiB/s" : "p50 ms");
    for (int k = 0; k < kLegs; ++k) {
        const double lo = *std::min_element(fig[k].begin(), fig[k].end());
        const double hi = *std::max_element(fig[k].begin(), fig[k].end());
        std::printf(", \"%s\": %s, \"%s_median\": %.3f, \"%s_range\": %.3f", kLegName[k], list(fig[k], scale).c_str(),
                    kLegName[k], pct(fig[k], 0.5) * scale, kLegName[k], (hi - lo) * scale);
        if (!burst) std::printf(", \"%s_p99_median\": %.3f", kLegName[k], pct(p99[k], 0.5) * 1e3);
    }
    std::printf(", \"A_over_B\": %.3f, \"zero_copy_slots\": %llu, \"gather_tiles\": %llu, \"wrong_verdicts\": %llu}\n",
                pct(fig[kHybrid], 0.5) / pct(fig[kPair], 0.5), (unsigned long long)st.zero_copy_slots,
                (unsigned long long)st.gather_tiles, (unsigned long long)p.wrong);
    return p.wrong == 0 ? 0 : 3;
}
