// vx_block_rounds.hpp — host-only round driver of the v2 and hybrid files calls
// (vx_merkle_files.hip, vx_hybrid.hip): the slot ring that reads round k + 1
// into one slot's pinned stage while the device works on round k.  No HIP in
// here: the ring runs on the CPU over a fake device (tests/native/block_rounds_check.cpp).
//
// Round k goes to slot k % nslots, in planner order.  A round carries no state
// of its slot, so a slot is free again as soon as its own round is done on the
// device, and reads run ahead as far as the slots allow: the round about to be
// enqueued may block on its slot's last round, read-ahead takes only a slot that
// is free now.  The caller's device answers three questions:
//   slots.done(si, block)    slot si's last round: 0 done, kNotYet (never when block), or an error
//   slots.stage(si, &rc)     slot si's pinned stage; rc 0 or an error
//   enqueue(si, round)       the round, read into that stage, onto the device; 0 or an error
// A planner has bool next(Round&); a Round has bytes, file_bytes and reads, each
// with file, file_off, len, piece and a stage_offset(read) beside its struct.
#pragma once
#include <vector>

#include "vx_files.hpp"

namespace vx_block_rounds {

constexpr int kNotYet = 1;
struct Totals {  // of the rounds enqueued; the last enqueue on Readers::now_ns's clock
    uint64_t rounds = 0, file_bytes = 0, copy_bytes = 0, last_enqueue_ns = vx_files::Readers::now_ns();
};

// Every round of `plan`; 0 or the device's first error, with no read
// outstanding either way (a copy may be: the caller drains its streams).
template <class Round, class Planner, class Slots, class Enqueue>
int run(Planner& plan, vx_files::Readers& rd, size_t nslots, Slots& slots, Enqueue&& enqueue, Totals& t) {
    std::vector<Round> round(nslots);
    std::vector<std::vector<vx_files::ReadItem>> items(nslots);  // unchanged until its ticket is waited for
    std::vector<uint64_t> ticket(nslots, 0);
    std::vector<uint8_t> live(nslots, 0);  // the slot carries an enqueued round
    const size_t depth = nslots - 1;
    bool more = true;
    size_t nr = 0;  // next round to read
    int rc = 0;
    for (size_t ne = 0; !rc; ++ne) {
        while (more && nr <= ne + depth && !rc) {
            const size_t si = nr % nslots;
            if (live[si]) {  // the round this slot carried: its stage and tables are free again after it
                const int q = slots.done(si, /*block=*/nr == ne);
                if (q == kNotYet) break;  // read-ahead takes only a slot that is free now
                if ((rc = q)) break;
                live[si] = 0;
            }
            if (!(more = plan.next(round[si]))) break;
            uint8_t* const stage = slots.stage(si, &rc);
            if (rc) break;
            items[si].clear();
            for (const auto& r : round[si].reads) {
                vx_files::ReadItem x{stage + stage_offset(r), r.piece, 0, r.len};
                x.file = (int32_t)r.file;
                x.file_off = (int64_t)r.file_off;
                items[si].push_back(x);
            }
            ticket[si] = rd.submit(items[si]);
            ++nr;
        }
        if (rc || ne == nr) break;
        const size_t si = ne % nslots;
        rd.wait(ticket[si]);
        if ((rc = enqueue(si, round[si]))) break;
        live[si] = 1;
        ++t.rounds;
        t.file_bytes += round[si].file_bytes;
        t.copy_bytes += round[si].bytes;
        t.last_enqueue_ns = vx_files::Readers::now_ns();
    }
    rd.wait();  // error path: no read may still target a stage
    return rc;
}

}  // namespace vx_block_rounds
