"""Shared by the file-hole tests (test_sparse_cpu.py, test_gpu_sparse.py):
sparse files made the ways a client makes them, and the probe that says
whether the test's file system reports holes at all."""
import errno
import os


def holes_reported(tmp_path) -> bool:
    """A truncate()d file must give ENXIO on SEEK_DATA; where it does not (a
    file system without hole reporting), assertions on hole counts do not
    apply.  Verdict assertions always do."""
    p = tmp_path / "hole_probe"
    with open(p, "wb") as f:
        f.truncate(1 << 20)
    fd = os.open(p, os.O_RDONLY)
    try:
        os.lseek(fd, 0, os.SEEK_DATA)
    except OSError as e:
        return e.errno == errno.ENXIO
    finally:
        os.close(fd)
    return False


NO_HOLES = "this file system reports no holes (SEEK_DATA on a truncated file gave no ENXIO)"


def make_file(path, length: int, writes=(), how: str = "truncate", size: int | None = None) -> str:
    """A file of `length` bytes made by truncate (what File::create + set_len
    leaves) or posix_fallocate (what FileStore::new does), then `writes`
    [(offset, bytes)] into it; size: its final size on disk when that differs
    (a file shorter than its torrent length)."""
    with open(path, "wb") as f:
        if how == "fallocate":
            if length:
                os.posix_fallocate(f.fileno(), 0, length)
        else:
            f.truncate(length)
        for off, data in writes:
            f.seek(off)
            f.write(data)
        if size is not None:
            f.truncate(size)
    return str(path)


def write_torrent_range(paths, file_lengths, lo: int, hi: int, data: bytes) -> None:
    """Write data[lo:hi] of the v1 torrent (the files laid end to end) into the
    files that hold it."""
    acc = 0
    for p, n in zip(paths, file_lengths):
        a, b = max(lo, acc), min(hi, acc + n)
        if a < b:
            with open(p, "r+b") as f:
                f.seek(a - acc)
                f.write(data[a:b])
        acc += n
