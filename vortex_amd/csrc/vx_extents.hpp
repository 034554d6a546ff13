// vx_extents.hpp — which bytes of the torrent's files were never written
// (DESIGN.md §6.11), host only: no HIP in here, the scan and the piece
// classification are tested on the CPU (tests/native/extents_dump.cpp).
//
// The reference re-verifies right after FileStore::new has fallocated every
// file to its torrent length (file_store.rs:22-43, :146; torrent.rs:716-761),
// so most of what a resume reads is zeros the file system makes up.  The file
// system knows: lseek(SEEK_DATA / SEEK_HOLE) walks a file's data extents, and
// what lies between them inside the file reads as zeros without being stored.
//
// Hole rule.  With bound = min(st_size, the file's torrent length):
//  * a byte is a hole byte iff its offset is below bound and in no data extent;
//  * bytes at or past st_size are missing, not holes: a short file fails the
//    pieces it fails without the scan, and they count as I/O errors as before;
//  * a file that did not open has no holes;
//  * ENXIO from SEEK_DATA means no data from there on; any other lseek error
//    makes the whole file data;
//  * at most `cap` extents are scanned per file; what lies beyond them is data.
#pragma once
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

#include <cerrno>
#include <cstdint>

#include <algorithm>
#include <vector>

#include "vx_files.hpp"

namespace vx_extents {

constexpr size_t kMaxExtents = 65536;

struct Extent {
    int64_t lo, hi;  // data bytes [lo, hi)
};

struct File {
    int64_t bound = 0;         // no byte at or past it is a hole
    std::vector<Extent> data;  // sorted, disjoint, inside [0, bound)
};

// The data extents of fd inside [0, min(st_size, length)).
inline File scan(int fd, uint64_t length, size_t cap = kMaxExtents) {
    File out;
    struct stat st;
    if (fd < 0 || fstat(fd, &st) != 0 || st.st_size <= 0) return out;  // nothing below the bound: no holes
    out.bound = (int64_t)std::min<uint64_t>((uint64_t)st.st_size, length);
    int64_t pos = 0;
    while (pos < out.bound) {
        if (out.data.size() >= cap) {  // past the cap: data
            out.data.push_back(Extent{pos, out.bound});
            break;
        }
        const off_t d = lseek(fd, (off_t)pos, SEEK_DATA);
        if (d < 0 && errno == ENXIO) break;  // a hole to the end of the file
        const off_t h = d < 0 ? (off_t)-1 : lseek(fd, d, SEEK_HOLE);
        if (d < 0 || h <= d) {  // the file system does not say: all data
            out.data.assign(1, Extent{0, out.bound});
            break;
        }
        if ((int64_t)d >= out.bound) break;
        out.data.push_back(Extent{(int64_t)d, std::min<int64_t>((int64_t)h, out.bound)});
        pos = (int64_t)h;
    }
    return out;
}

class Holes {
  public:
    Holes() = default;
    // Scans every opened file (fds[f] < 0: not opened, no holes).
    Holes(const std::vector<int>& fds, const uint64_t* file_lengths, size_t cap = kMaxExtents) : files_(fds.size()) {
        for (size_t f = 0; f < fds.size(); ++f) {
            files_[f] = scan(fds[f], file_lengths[f], cap);
            extents_ += files_[f].data.size();
            uint64_t data = 0;
            for (const Extent& e : files_[f].data) data += (uint64_t)(e.hi - e.lo);
            any_ |= (uint64_t)files_[f].bound > data;
        }
    }
    bool any() const { return any_; }  // some byte of some file is a hole byte
    uint64_t extents() const { return extents_; }
    const File& file(size_t f) const { return files_[f]; }

    // Every byte of [off, off + len) of file f is a hole byte (len > 0).
    bool hole(uint32_t f, int64_t off, int64_t len) const {
        if (f >= files_.size() || len <= 0 || off < 0) return false;
        const File& x = files_[f];
        if (off + len > x.bound) return false;
        // the first extent that ends past off: a hole range meets none
        auto it = std::upper_bound(x.data.begin(), x.data.end(), off,
                                   [](int64_t o, const Extent& e) { return o < e.hi; });
        return it == x.data.end() || it->lo >= off + len;
    }

    // v1: piece `piece` is a hole piece when it has bytes and every one of its
    // segments (vx_files::segments, into segs) lies wholly in holes.
    bool hole_piece(const std::vector<vx_files::FileSpan>& fs, int64_t piece, uint32_t piece_length,
                    std::vector<vx_files::Seg>& segs) const {
        vx_files::segments(fs, piece, piece_length, segs);
        for (const vx_files::Seg& s : segs)
            if (!hole(s.file, s.off, s.len)) return false;
        return !segs.empty();
    }

  private:
    std::vector<File> files_;
    uint64_t extents_ = 0;
    bool any_ = false;
};

}  // namespace vx_extents
