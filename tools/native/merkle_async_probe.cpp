// merkle_async_probe.cpp — the download path for v1 (vx_submit, SHA-1) and v2
// (vx_merkle_submit, SHA-256 merkle) pieces side by side: one process, one
// context, the same registered buffers (one mmap per buffer, as vortex's
// BufferPool has, buf_pool.rs:92-98), legs of the two kinds alternating so
// both see the same machine state.
//
//   burst  every buffer submitted once as fast as vx_submit takes them, then
//          flushed and polled dry: GiB/s of `total` bytes per leg.
//   loop   the event loop's shape: `batch` pieces submitted, one vx_flush,
//          then vx_poll until all are back; per piece the time from its
//          submit to the poll that returned it: p50 / p99 per leg.
//
// Every verdict is checked (expected digests and roots come from the bulk
// calls first; every 97th is planted wrong).  Prints one JSON line with each
// leg's figure and the medians.
//
// A last argument `zc` adds a third kind of leg: v2 with vx_set_merkle_zero_copy
// on (the slots hashed straight out of the registered buffers), alternating
// with the v1 legs and the gathered v2 legs in the same process; its figures
// are the "v2zc_" keys and the trace of vx_merkle_zero_copy_trace.
//
// usage: merkle_async_probe burst <piece_len> [total_bytes=2147483648] [reps=5] [zc]
//        merkle_async_probe loop  <piece_len> [batch=32] [batches=200] [reps=5] [zc]
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

struct Probe {
    vx_ctx* ctx = nullptr;
    uint32_t plen = 0, log2w = 0, nbuf = 0;
    std::vector<uint8_t*> bufs;
    std::vector<uint8_t> sha1, roots;  // expected rows, every 97th wrong
    std::vector<clk::time_point> t_sub;
    std::vector<vx_completion> cq1{4096};
    std::vector<vx_merkle_completion> cq2{4096};
    uint64_t wrong = 0;

    int submit(bool v2, uint32_t b) {
        t_sub[b] = clk::now();
        return v2 ? vx_merkle_submit(ctx, b, bufs[b], plen, log2w, &roots[(size_t)b * 32])
                  : vx_submit(ctx, b, bufs[b], plen, &sha1[(size_t)b * 20]);
    }
    // Completions of one kind polled once; their latencies appended to lat (if given).
    int64_t poll(bool v2, std::vector<double>* lat) {
        const int64_t k = v2 ? vx_merkle_poll(ctx, cq2.data(), cq2.size()) : vx_poll(ctx, cq1.data(), cq1.size());
        const auto now = clk::now();
        for (int64_t j = 0; j < k; ++j) {
            const uint32_t b = (uint32_t)(v2 ? cq2[j].tag : cq1[j].tag);
            const bool matched = (v2 ? cq2[j].matched : cq1[j].matched) != 0;
            wrong += matched != (b % 97 != 0);
            if (lat) lat->push_back(since(t_sub[b], now));
        }
        return k;
    }
};

int main(int argc, char** argv) {
    if (argc < 3 || (std::strcmp(argv[1], "burst") && std::strcmp(argv[1], "loop"))) {
        std::fprintf(stderr, "usage: %s burst piece_len [total_bytes] [reps]\n       %s loop piece_len [batch] [batches] [reps]\n",
                     argv[0], argv[0]);
        return 2;
    }
    const bool burst = !std::strcmp(argv[1], "burst");
    const bool zc = !std::strcmp(argv[argc - 1], "zc");
    if (zc) --argc;
    const int kinds = zc ? 3 : 2;  // 0: v1, 1: v2 gathered, 2: v2 zero-copy
    Probe p;
    p.plen = (uint32_t)std::strtoul(argv[2], nullptr, 0);
    const uint64_t total = burst && argc > 3 ? std::strtoull(argv[3], nullptr, 0) : 2ull << 30;
    const uint32_t batch = !burst && argc > 3 ? (uint32_t)std::atoi(argv[3]) : 32;
    const uint32_t batches = !burst && argc > 4 ? (uint32_t)std::atoi(argv[4]) : 200;
    const int reps = std::max(1, argc > (burst ? 4 : 5) ? std::atoi(argv[burst ? 4 : 5]) : 5);
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
    std::mt19937_64 rng(p.plen ^ 0xB52);
    p.bufs.resize(p.nbuf);
    p.t_sub.resize(p.nbuf);
    std::vector<const uint8_t*> ptrs(p.nbuf);
    std::vector<uint32_t> lens(p.nbuf, p.plen);
    for (uint32_t b = 0; b < p.nbuf; ++b) {
        void* m = mmap(nullptr, p.plen, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_POPULATE, -1, 0);
        if (m == MAP_FAILED) return 1;
        p.bufs[b] = static_cast<uint8_t*>(m);
        ptrs[b] = p.bufs[b];
        for (size_t i = 0; i < p.plen / 8; ++i) reinterpret_cast<uint64_t*>(p.bufs[b])[i] = rng();
        if (int rc = vx_register_host_buffer(p.ctx, p.bufs[b], p.plen)) {
            std::fprintf(stderr, "register: %d %s\n", rc, vx_last_error());
            return 1;
        }
    }
    // the expected rows, from the bulk calls (tested against hashlib elsewhere)
    p.sha1.resize((size_t)p.nbuf * 20);
    p.roots.resize((size_t)p.nbuf * 32);
    std::vector<uint8_t> zeros((size_t)p.nbuf * 32), verdicts(p.nbuf);
    int rc = vx_sha1_batch(p.ctx, ptrs.data(), lens.data(), p.nbuf, p.sha1.data());
    if (!rc)
        rc = vx_merkle_verify_batch(p.ctx, ptrs.data(), lens.data(), nullptr, p.nbuf, p.plen, zeros.data(),
                                    verdicts.data(), p.roots.data());
    if (rc) {
        std::fprintf(stderr, "expected rows: %d %s\n", rc, vx_last_error());
        return 1;
    }
    for (uint32_t b = 0; b < p.nbuf; b += 97) {
        p.sha1[(size_t)b * 20 + 3] ^= 1;
        p.roots[(size_t)b * 32 + 3] ^= 1;
    }

    // One leg: `rounds` times submit every buffer, flush, poll until all are back.
    auto leg = [&](bool v2, uint32_t rounds, std::vector<double>* lat, double* seconds) -> int {
        const auto t0 = clk::now();
        for (uint32_t r = 0; r < rounds; ++r) {
            for (uint32_t b = 0; b < p.nbuf; ++b)
                if (int e = p.submit(v2, b)) return e;
            if (int e = vx_flush(p.ctx)) return e;
            for (uint64_t got = 0; got < p.nbuf;) {
                const int64_t k = p.poll(v2, lat);
                if (k < 0) return (int)k;
                got += (uint64_t)k;
                if (since(t0, clk::now()) > 120) return VX_EBUSY;  // never in practice: a stuck batch
            }
        }
        *seconds = since(t0, clk::now());
        return 0;
    };
    const uint32_t rounds = burst ? 1 : batches;
    std::vector<double> fig[3], p99[3];  // per kind: GiB/s (burst) or p50 seconds (loop)
    double s = 0;
    auto kind_leg = [&](int kind, uint32_t n_rounds, std::vector<double>* lat) -> int {
        if (zc)
            if (int e = vx_set_merkle_zero_copy(p.ctx, kind == 2)) return e;
        return leg(kind != 0, n_rounds, lat, &s);
    };
    for (int k = 0; k < kinds && !rc; ++k) rc = kind_leg(k, burst ? 1 : 8, nullptr);  // warm every kind's buffers
    for (int r = 0; r < reps && !rc; ++r) {
        for (int k = 0; k < kinds && !rc; ++k) {
            std::vector<double> lat;
            rc = kind_leg(k, rounds, &lat);
            if (burst) {
                fig[k].push_back((double)p.nbuf * p.plen / s / (double)(1ull << 30));
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
    vx_merkle_zc_trace tr{};
    vx_merkle_zero_copy_trace(p.ctx, &tr);
    char zcs[512] = "";
    if (zc && burst)
        std::snprintf(zcs, sizeof zcs, ", \"v2zc_GiBps\": %s, \"v2zc_GiBps_median\": %.3f, \"v2zc_over_v2\": %.3f, "
                      "\"zc_trace\": {\"slots\": %llu, \"pieces\": %llu, \"bytes\": %llu, \"fallback_slots\": %llu}",
                      list(fig[2], 1).c_str(), pct(fig[2], 0.5), pct(fig[2], 0.5) / pct(fig[1], 0.5),
                      (unsigned long long)tr.slots, (unsigned long long)tr.pieces, (unsigned long long)tr.bytes,
                      (unsigned long long)tr.fallback_slots);
    else if (zc)
        std::snprintf(zcs, sizeof zcs, ", \"v2zc_p50_ms\": %s, \"v2zc_p99_ms\": %s, \"v2zc_p50_ms_median\": %.3f, "
                      "\"v2zc_p99_ms_median\": %.3f, \"v2zc_over_v2_p50\": %.3f, "
                      "\"zc_trace\": {\"slots\": %llu, \"pieces\": %llu, \"bytes\": %llu, \"fallback_slots\": %llu}",
                      list(fig[2], 1e3).c_str(), list(p99[2], 1e3).c_str(), pct(fig[2], 0.5) * 1e3,
                      pct(p99[2], 0.5) * 1e3, pct(fig[2], 0.5) / pct(fig[1], 0.5), (unsigned long long)tr.slots,
                      (unsigned long long)tr.pieces, (unsigned long long)tr.bytes,
                      (unsigned long long)tr.fallback_slots);
    for (uint32_t b = 0; b < p.nbuf; ++b) {
        vx_unregister_host_buffer(p.ctx, p.bufs[b]);
        munmap(p.bufs[b], p.plen);
    }
    vx_destroy(p.ctx);
    if (burst) {
        std::printf("{\"mode\": \"burst\", \"piece_len\": %u, \"pieces\": %u, \"bytes\": %llu, \"reps\": %d, "
                    "\"v1_GiBps\": %s, \"v2_GiBps\": %s, \"v1_GiBps_median\": %.3f, \"v2_GiBps_median\": %.3f, "
                    "\"v2_over_v1\": %.3f, \"zero_copy_slots\": %llu, \"gather_tiles\": %llu, \"wrong_verdicts\": %llu%s}\n",
                    p.plen, p.nbuf, (unsigned long long)p.nbuf * p.plen, reps, list(fig[0], 1).c_str(),
                    list(fig[1], 1).c_str(), pct(fig[0], 0.5), pct(fig[1], 0.5), pct(fig[1], 0.5) / pct(fig[0], 0.5),
                    (unsigned long long)st.zero_copy_slots, (unsigned long long)st.gather_tiles,
                    (unsigned long long)p.wrong, zcs);
    } else {
        std::printf("{\"mode\": \"loop\", \"piece_len\": %u, \"batch\": %u, \"batches_per_leg\": %u, \"reps\": %d, "
                    "\"v1_p50_ms\": %s, \"v2_p50_ms\": %s, \"v1_p99_ms\": %s, \"v2_p99_ms\": %s, "
                    "\"v1_p50_ms_median\": %.3f, \"v2_p50_ms_median\": %.3f, \"v1_p99_ms_median\": %.3f, "
                    "\"v2_p99_ms_median\": %.3f, \"v2_over_v1_p50\": %.3f, \"wrong_verdicts\": %llu%s}\n",
                    p.plen, batch, batches, reps, list(fig[0], 1e3).c_str(), list(fig[1], 1e3).c_str(),
                    list(p99[0], 1e3).c_str(), list(p99[1], 1e3).c_str(), pct(fig[0], 0.5) * 1e3,
                    pct(fig[1], 0.5) * 1e3, pct(p99[0], 0.5) * 1e3, pct(p99[1], 0.5) * 1e3,
                    pct(fig[1], 0.5) / pct(fig[0], 0.5), (unsigned long long)p.wrong, zcs);
    }
    return p.wrong == 0 ? 0 : 3;
}
