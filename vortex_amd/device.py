"""Device-resident batch API (the hot path): torch tensors in, digests out.

PyTorch is only plumbing here — it owns the HBM allocations and the stream;
the hashing is the HIP kernels in libvortex_amd.so, called through the C ABI
(``vx_sha1_device_uniform`` / ``vx_sha1_device_ragged``).

Layout (DESIGN.md "Data layout in HBM"): one uint8 tensor holds all pieces;
piece i starts at ``i * stride`` (uniform) or ``offsets[i]`` (ragged), every
start 16-byte aligned.  Digests are ``[n, 20]`` uint8 (big-endian SHA-1),
verdicts ``[n]`` uint8 (0/1).
"""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import check, lib, tuning


def _stream_ptr(stream: Optional[torch.cuda.Stream], device: torch.device) -> int:
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return int(s.cuda_stream)


def _req(t: torch.Tensor, name: str, dtype=torch.uint8) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def sha1_uniform(data: torch.Tensor, n: int, piece_len: int, stride: Optional[int] = None,
                 expected: Optional[torch.Tensor] = None, digests: Optional[torch.Tensor] = None,
                 matched: Optional[torch.Tensor] = None, want_digests: bool = True,
                 stream: Optional[torch.cuda.Stream] = None, variant: int = 0):
    """Hash n pieces of piece_len bytes at data[i*stride : i*stride+piece_len].

    Returns (digests [n,20] or None, matched [n] or None).  Enqueue-only.
    variant: 0 = the default kernel (vx_sha1_device_uniform, the release
    library); others pin a variant through the tuning build (vx_tuning.h)."""
    _req(data, "data")
    stride = piece_len if stride is None else stride
    if n and (n - 1) * stride + piece_len > data.numel():
        raise ValueError("batch exceeds data tensor")
    dev = data.device
    if want_digests and digests is None:
        digests = torch.empty((n, 20), dtype=torch.uint8, device=dev)
    elif want_digests:
        _req(digests, "digests")
        if digests.numel() < 20 * n or digests.device != dev:
            raise ValueError("digests must hold n*20 bytes on the data's device")
    if expected is not None:
        _req(expected, "expected")
        if expected.numel() < 20 * n or expected.device != dev:
            raise ValueError("expected must hold n*20 bytes on the data's device")
        if matched is None:
            matched = torch.empty((n,), dtype=torch.uint8, device=dev)
        else:
            _req(matched, "matched")
            if matched.numel() < n or matched.device != dev:
                raise ValueError("matched must hold n bytes on the data's device")
    args = (data.data_ptr(), stride, piece_len, n,
            digests.data_ptr() if (want_digests and digests is not None) else None,
            expected.data_ptr() if expected is not None else None,
            matched.data_ptr() if expected is not None else None,
            _stream_ptr(stream, dev))
    if variant == 0:
        check(lib().vx_sha1_device_uniform(*args), "vx_sha1_device_uniform")
    else:
        check(tuning().vx_sha1_device_uniform_variant(*args, variant), "vx_sha1_device_uniform_variant", tuning())
    return (digests if want_digests else None), (matched if expected is not None else None)


def _check_ragged_layout(data: torch.Tensor, offsets: torch.Tensor, lens: torch.Tensor,
                         order: Optional[torch.Tensor]) -> None:
    """The kernels trust their offsets (vx_hash.h: the raw device entries do
    not validate device-resident metadata), so check here what an
    out-of-range batch would otherwise turn into reads of arbitrary HBM:
    every offset 16-byte aligned and >= 0, every length >= 0, every piece
    inside `data`, and `order` a set of indices in [0, n).  One small
    reduction on the device and one 4-value copy back (a sync)."""
    n = offsets.numel()
    if n == 0:
        return
    ends = offsets + lens.to(torch.int64)
    stats = torch.stack([
        (offsets & 15).ne(0).any().to(torch.int64),
        offsets.min().lt(0).to(torch.int64) + lens.min().lt(0).to(torch.int64),
        ends.max(),
        (order.min().lt(0) | order.max().ge(n)).to(torch.int64) if order is not None else offsets.new_zeros(()),
    ]).cpu().tolist()
    if stats[0]:
        raise ValueError("sha1_ragged: every offset must be a multiple of 16 (the kernels load 16 bytes per lane)")
    if stats[1]:
        raise ValueError("sha1_ragged: negative offset or length")
    if stats[2] > data.numel():
        raise ValueError(f"sha1_ragged: a piece ends at byte {stats[2]}, past the data tensor ({data.numel()} bytes)")
    if stats[3]:
        raise ValueError("sha1_ragged: order holds an index outside [0, n)")


def sha1_ragged(data: torch.Tensor, offsets: torch.Tensor, lens: torch.Tensor,
                order: Optional[torch.Tensor] = None, expected: Optional[torch.Tensor] = None,
                digests: Optional[torch.Tensor] = None, matched: Optional[torch.Tensor] = None,
                stream: Optional[torch.cuda.Stream] = None, variant: int = 0, plan=None,
                validate: bool = True):
    """Hash piece i = data[offsets[i] : offsets[i]+lens[i]] for all i.

    offsets: int64 device tensor (16-byte aligned values); lens: int32 device
    tensor; order: optional int32 permutation (see :func:`length_order`).
    variant: 0 = default kernel; 1 lane / 2 split pin one (vx_tuning.h).
    plan: (max_len, total_bytes) of the batch, known on the host when it is
    laid out (see :func:`ragged_plan`); with variant 0 the engine then picks
    the kernel whose time bound is lower (vx_sha1_device_ragged_hint,
    DESIGN.md §3.4).
    validate: check alignment and bounds of offsets/lens/order first (a
    device reduction and a sync; see :func:`_check_ragged_layout`).  Pass
    False only for a layout built by trusted code, e.g. a timed loop over a
    batch that was validated once."""
    _req(data, "data")
    _req(offsets, "offsets", torch.int64)
    _req(lens, "lens", torch.int32)
    n = offsets.numel()
    if lens.numel() != n:
        raise ValueError("offsets and lens differ in length")
    if order is not None:
        _req(order, "order", torch.int32)
        if order.numel() != n:
            raise ValueError("order must hold n indices")
    dev = data.device
    for name, t in (("offsets", offsets), ("lens", lens), ("order", order), ("expected", expected),
                    ("digests", digests), ("matched", matched)):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, data on {dev}")
    if validate:
        _check_ragged_layout(data, offsets, lens, order)
    if digests is None:
        digests = torch.empty((n, 20), dtype=torch.uint8, device=dev)
    elif digests.dtype != torch.uint8 or not digests.is_contiguous() or digests.numel() < 20 * n:
        raise ValueError("digests must be a contiguous uint8 tensor of n*20 bytes")
    if expected is not None:
        _req(expected, "expected")
        if expected.numel() < 20 * n:
            raise ValueError("expected must hold n*20 bytes")
        if matched is None:
            matched = torch.empty((n,), dtype=torch.uint8, device=dev)
        elif matched.dtype != torch.uint8 or not matched.is_contiguous() or matched.numel() < n:
            raise ValueError("matched must be a contiguous uint8 tensor of n bytes")
    exp_p = expected.data_ptr() if expected is not None else None
    m_p = matched.data_ptr() if expected is not None else None
    order_p = order.data_ptr() if order is not None else None
    if variant == 0 and plan is not None:
        max_len, total = plan
        rc = lib().vx_sha1_device_ragged_hint(data.data_ptr(), offsets.data_ptr(), lens.data_ptr(), order_p, n,
                                              int(max_len), int(total), digests.data_ptr(), exp_p, m_p,
                                              _stream_ptr(stream, dev))
        check(rc, "vx_sha1_device_ragged_hint")
    elif variant == 0:
        rc = lib().vx_sha1_device_ragged(data.data_ptr(), offsets.data_ptr(), lens.data_ptr(), order_p, n,
                                         digests.data_ptr(), exp_p, m_p, _stream_ptr(stream, dev))
        check(rc, "vx_sha1_device_ragged")
    else:
        rc = tuning().vx_sha1_device_ragged_variant(data.data_ptr(), offsets.data_ptr(), lens.data_ptr(), order_p, n,
                                                    digests.data_ptr(), exp_p, m_p, _stream_ptr(stream, dev), variant)
        check(rc, "vx_sha1_device_ragged_variant", tuning())
    return digests, matched


def _merkle_outputs(n: int, log2_width: int, dev, expected, leaves, roots, matched, want_leaves: bool = True):
    """Allocate / check the output tensors of a merkle call (want_leaves
    False: a call that keeps no leaf layer; `leaves` comes back as given)."""
    if not 0 <= log2_width <= 17:
        raise ValueError("log2_width must be 0..17")
    rows = n << log2_width
    if rows >> 32:
        raise ValueError("n << log2_width must fit 32 bits")
    if not want_leaves:
        pass
    elif leaves is None:
        leaves = torch.empty((rows, 32), dtype=torch.uint8, device=dev)
    else:
        _req(leaves, "leaves")
        if leaves.numel() < 32 * rows or leaves.device != dev:
            raise ValueError("leaves must hold (n << log2_width)*32 bytes on the data's device")
    if roots is None:
        roots = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    else:
        _req(roots, "roots")
        if roots.numel() < 32 * n or roots.device != dev:
            raise ValueError("roots must hold n*32 bytes on the data's device")
    if expected is not None:
        _req(expected, "expected")
        if expected.numel() < 32 * n or expected.device != dev:
            raise ValueError("expected must hold n*32 bytes on the data's device")
        if matched is None:
            matched = torch.empty((n,), dtype=torch.uint8, device=dev)
        else:
            _req(matched, "matched")
            if matched.numel() < n or matched.device != dev:
                raise ValueError("matched must hold n bytes on the data's device")
    else:
        matched = None
    return leaves, roots, matched


def merkle_uniform(data: torch.Tensor, n: int, piece_len: int, log2_width: int, stride: Optional[int] = None,
                   last_len: Optional[int] = None, expected: Optional[torch.Tensor] = None,
                   leaves: Optional[torch.Tensor] = None, roots: Optional[torch.Tensor] = None,
                   matched: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None):
    """BitTorrent v2 roots of n pieces at data[i*stride : i*stride+piece_len]
    (the last one last_len bytes), each a SHA-256 merkle tree of
    2^log2_width 16 KiB leaf slots (vx_merkle_device_uniform).

    Returns (roots [n,32], leaves [n << log2_width, 32], matched [n] or None).
    Every leaf row is written, zero rows included.  Enqueue-only."""
    _req(data, "data")
    stride = piece_len if stride is None else stride
    last_len = piece_len if last_len is None else last_len
    if n and (n - 1) * stride + last_len > data.numel():
        raise ValueError("batch exceeds data tensor")
    dev = data.device
    leaves, roots, matched = _merkle_outputs(n, log2_width, dev, expected, leaves, roots, matched)
    rc = lib().vx_merkle_device_uniform(data.data_ptr(), stride, piece_len, last_len, n, log2_width,
                                        leaves.data_ptr(), roots.data_ptr(),
                                        expected.data_ptr() if expected is not None else None,
                                        matched.data_ptr() if matched is not None else None,
                                        _stream_ptr(stream, dev))
    check(rc, "vx_merkle_device_uniform")
    return roots, leaves, matched


def _check_merkle_layout(data: torch.Tensor, offsets: torch.Tensor, lens: torch.Tensor,
                         log2w: Optional[torch.Tensor], log2_width: int, who: str = "merkle_ragged") -> None:
    """What :func:`_check_ragged_layout` checks for sha1_ragged, for a merkle
    batch: offsets 16-byte aligned and >= 0, lengths >= 0, every piece inside
    `data`, every log2w <= log2_width and every piece inside its own tree
    (16384 << log2w bytes).  One device reduction and one copy back (a sync).

    `lens` is int32 here, so a piece is at most 2^31 - 1 bytes.  The C entries
    take uint32 lengths, and exactly one length above that is valid there: 2^31,
    the full 2 GiB piece of a tree of 2^17 slots.  This module refuses it: its
    bits in an int32 tensor are a negative length, and the ValueError says so."""
    if offsets.numel() == 0:
        return
    ends = offsets + lens.to(torch.int64)
    lw = log2w.to(torch.int64) if log2w is not None else torch.full_like(offsets, log2_width)
    stats = torch.stack([
        (offsets & 15).ne(0).any().to(torch.int64),
        offsets.min().lt(0).to(torch.int64) + lens.min().lt(0).to(torch.int64),
        ends.max(),
        lw.max(),
        (lens.to(torch.int64) > torch.bitwise_left_shift(torch.full_like(lw, 16384), lw.clamp(0, 17))).any().to(torch.int64),
    ]).cpu().tolist()
    if stats[0]:
        raise ValueError(f"{who}: every offset must be a multiple of 16 (the kernels load 16 bytes per lane)")
    if stats[1]:
        raise ValueError(f"{who}: negative offset or length (lens is int32: a piece of 2^31 bytes, the full tree of "
                         "2^17 slots, has no length here and is refused)")
    if stats[2] > data.numel():
        raise ValueError(f"{who}: a piece ends at byte {stats[2]}, past the data tensor "
                         f"({data.numel()} bytes)")
    if stats[3] > log2_width:
        raise ValueError(f"{who}: log2w {stats[3]} > log2_width {log2_width}")
    if stats[4]:
        raise ValueError(f"{who}: a piece is longer than its tree (16384 << log2w bytes)")


def merkle_ragged(data: torch.Tensor, offsets: torch.Tensor, lens: torch.Tensor, log2_width: int,
                  log2w: Optional[torch.Tensor] = None, expected: Optional[torch.Tensor] = None,
                  leaves: Optional[torch.Tensor] = None, roots: Optional[torch.Tensor] = None,
                  matched: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                  validate: bool = True):
    """BitTorrent v2 roots of piece i = data[offsets[i] : offsets[i]+lens[i]]
    (vx_merkle_device_ragged).  offsets: int64 device tensor (16-byte aligned
    values); lens: int32; log2w: optional uint8, piece i's own tree width
    (<= log2_width; merkle.file_pieces).  Piece i's leaf rows start at row
    i << log2_width whatever its log2w.  validate: as for :func:`sha1_ragged`.
    log2_width goes up to 17; lens being int32, a piece is at most 2^31 - 1
    bytes, and the full 2^31-byte piece of width 17 is refused
    (:func:`_check_merkle_layout`; the same holds for merkle_pieces,
    merkle_block_check and hybrid_pieces).

    Returns (roots [n,32], leaves [n << log2_width, 32], matched [n] or None)."""
    _req(data, "data")
    _req(offsets, "offsets", torch.int64)
    _req(lens, "lens", torch.int32)
    n = offsets.numel()
    if lens.numel() != n:
        raise ValueError("offsets and lens differ in length")
    if log2w is not None:
        _req(log2w, "log2w")
        if log2w.numel() != n:
            raise ValueError("log2w must hold n widths")
    dev = data.device
    for name, t in (("offsets", offsets), ("lens", lens), ("log2w", log2w)):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, data on {dev}")
    leaves, roots, matched = _merkle_outputs(n, log2_width, dev, expected, leaves, roots, matched)
    if validate:
        _check_merkle_layout(data, offsets, lens, log2w, log2_width)
    rc = lib().vx_merkle_device_ragged(data.data_ptr(), offsets.data_ptr(), lens.data_ptr(),
                                       log2w.data_ptr() if log2w is not None else None, n, log2_width,
                                       leaves.data_ptr(), roots.data_ptr(),
                                       expected.data_ptr() if expected is not None else None,
                                       matched.data_ptr() if matched is not None else None,
                                       _stream_ptr(stream, dev))
    check(rc, "vx_merkle_device_ragged")
    return roots, leaves, matched


def merkle_pieces(data: torch.Tensor, offsets: torch.Tensor, lens: torch.Tensor, log2_width: int,
                  log2w: Optional[torch.Tensor] = None, expected: Optional[torch.Tensor] = None,
                  roots: Optional[torch.Tensor] = None, matched: Optional[torch.Tensor] = None,
                  stream: Optional[torch.cuda.Stream] = None, validate: bool = True):
    """The batch of :func:`merkle_ragged` through the fused piece kernel
    (vx_merkle_device_pieces), which keeps no leaf layer: the leaf rows are
    reduced in LDS.  One launch for log2_width <= 8; above, a work tensor of
    (n << (log2_width - 8)) * 32 + n bytes is allocated here and a node launch
    follows.  Arguments and layout checks as for merkle_ragged.

    Returns (roots [n,32], matched [n] or None)."""
    _req(data, "data")
    _req(offsets, "offsets", torch.int64)
    _req(lens, "lens", torch.int32)
    n = offsets.numel()
    if lens.numel() != n:
        raise ValueError("offsets and lens differ in length")
    if log2w is not None:
        _req(log2w, "log2w")
        if log2w.numel() != n:
            raise ValueError("log2w must hold n widths")
    dev = data.device
    for name, t in (("offsets", offsets), ("lens", lens), ("log2w", log2w)):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, data on {dev}")
    _, roots, matched = _merkle_outputs(n, log2_width, dev, expected, None, roots, matched, want_leaves=False)
    if validate:
        _check_merkle_layout(data, offsets, lens, log2w, log2_width, "merkle_pieces")
    work = None
    if log2_width > 8 and n:
        work = torch.empty(((n << (log2_width - 8)) * 32 + n,), dtype=torch.uint8, device=dev)
        if stream is not None:  # the scratch outlives this call on the stream that uses it
            work.record_stream(stream)
    rc = lib().vx_merkle_device_pieces(data.data_ptr(), offsets.data_ptr(), lens.data_ptr(),
                                       log2w.data_ptr() if log2w is not None else None, n, log2_width,
                                       work.data_ptr() if work is not None else None, roots.data_ptr(),
                                       expected.data_ptr() if expected is not None else None,
                                       matched.data_ptr() if matched is not None else None,
                                       _stream_ptr(stream, dev))
    check(rc, "vx_merkle_device_pieces")
    return roots, matched


def merkle_block_check(data: torch.Tensor, offsets: torch.Tensor, lens: torch.Tensor, log2_width: int,
                       expected_leaves: Optional[torch.Tensor] = None, leaves: Optional[torch.Tensor] = None,
                       stream: Optional[torch.cuda.Stream] = None, bad: Optional[torch.Tensor] = None,
                       want_leaves: Optional[bool] = None, validate: bool = True):
    """Check the batch of :func:`merkle_ragged` (every piece a tree of
    2^log2_width slots) block by block (vx_merkle_device_block_check):
    expected_leaves holds the (n << log2_width) * 32 bytes a merkle_ragged call
    on good data writes to `leaves`.  One launch.

    Returns (bad, leaves).  bad: int64 [merkle.bitmap_words(n, log2_width)], the
    bitmap's uint64 words bit for bit (torch has little arithmetic for uint64;
    ``bad.cpu().numpy().view("uint64")``): block b of piece i is bit b & 63 of
    word i * max(1, 2^log2_width / 64) + (b >> 6).  Every word is written; a
    slot at or past a piece's end is never set.  None without expected_leaves.
    leaves: the leaf rows [n << log2_width, 32], kept when `leaves` is given or
    want_leaves is true (the default without expected_leaves), else None.
    Layout checks (validate) as for merkle_ragged."""
    _req(data, "data")
    _req(offsets, "offsets", torch.int64)
    _req(lens, "lens", torch.int32)
    n = offsets.numel()
    if lens.numel() != n:
        raise ValueError("offsets and lens differ in length")
    if not 0 <= log2_width <= 17:
        raise ValueError("log2_width must be 0..17")
    rows = n << log2_width
    if rows >> 32:
        raise ValueError("n << log2_width must fit 32 bits")
    dev = data.device
    for name, t in (("offsets", offsets), ("lens", lens), ("expected_leaves", expected_leaves), ("leaves", leaves),
                    ("bad", bad)):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, data on {dev}")
    if want_leaves is None:
        want_leaves = leaves is not None or expected_leaves is None
    if expected_leaves is None and not want_leaves:
        raise ValueError("merkle_block_check: neither expected_leaves nor leaves asked for")
    words = n * max(1, (1 << log2_width) // 64)
    if expected_leaves is not None:
        _req(expected_leaves, "expected_leaves")
        if expected_leaves.numel() < 32 * rows:
            raise ValueError("expected_leaves must hold (n << log2_width)*32 bytes")
        if bad is None:
            bad = torch.empty((words,), dtype=torch.int64, device=dev)
        else:
            _req(bad, "bad", torch.int64)
            if bad.numel() < words:
                raise ValueError("bad must hold merkle.bitmap_words(n, log2_width) words")
    elif bad is not None:
        raise ValueError("bad needs expected_leaves")
    if not want_leaves:
        leaves = None
    elif leaves is None:
        leaves = torch.empty((rows, 32), dtype=torch.uint8, device=dev)
    else:
        _req(leaves, "leaves")
        if leaves.numel() < 32 * rows:
            raise ValueError("leaves must hold (n << log2_width)*32 bytes")
    if validate:
        _check_merkle_layout(data, offsets, lens, None, log2_width, "merkle_block_check")
    rc = lib().vx_merkle_device_block_check(data.data_ptr(), offsets.data_ptr(), lens.data_ptr(), n, log2_width,
                                            expected_leaves.data_ptr() if expected_leaves is not None else None,
                                            bad.data_ptr() if bad is not None else None,
                                            leaves.data_ptr() if leaves is not None else None,
                                            _stream_ptr(stream, dev))
    check(rc, "vx_merkle_device_block_check")
    return bad, leaves


def hybrid_work_bytes(n: int, log2_width: int) -> int:
    """Bytes of the work tensor of :func:`hybrid_pieces` (vx_hash.h,
    vx_hybrid_device_pieces): the merkle piece kernel's work rounded up to 16,
    then 54 bytes per piece."""
    w = ((n << (log2_width - 8)) * 32 + n + 15) // 16 * 16 if log2_width > 8 else 0
    return w + 54 * n


def hybrid_pieces(data: torch.Tensor, offsets: torch.Tensor, lens: torch.Tensor, pads: torch.Tensor,
                  log2_width: int, log2w: Optional[torch.Tensor] = None, exp_sha1: Optional[torch.Tensor] = None,
                  exp_roots: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                  validate: bool = True):
    """The pieces of a hybrid (v1 + v2) torrent in one call over one buffer
    (vx_hybrid_device_pieces): piece i is data[offsets[i] : offsets[i] +
    lens[i]], its v1 digest is over those bytes followed by pads[i] zeros that
    exist nowhere (pads[i] is 0 or (16384 << log2_width) - lens[i]; see
    vortex_amd.hybrid.hybrid_pieces), its v2 root over the bytes alone as a
    tree of 2^log2w[i] leaf slots.  offsets int64, lens and pads int32, log2w
    uint8 device tensors; exp_sha1 [n,20] and exp_roots [n,32] uint8 or None.

    Returns (sha1 [n,20], roots [n,32], matched [n] or None); matched has bit
    0 set where the SHA-1 matches and bit 1 where the root does, and is None
    when neither expected table is given.  Enqueue-only."""
    _req(data, "data")
    _req(offsets, "offsets", torch.int64)
    _req(lens, "lens", torch.int32)
    _req(pads, "pads", torch.int32)
    n = offsets.numel()
    if lens.numel() != n or pads.numel() != n:
        raise ValueError("offsets, lens and pads differ in length")
    if log2w is not None:
        _req(log2w, "log2w")
        if log2w.numel() != n:
            raise ValueError("log2w must hold n widths")
    dev = data.device
    for name, t, row in (("offsets", offsets, 0), ("lens", lens, 0), ("pads", pads, 0), ("log2w", log2w, 0),
                         ("exp_sha1", exp_sha1, 20), ("exp_roots", exp_roots, 32)):
        if t is None:
            continue
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, data on {dev}")
        if row:
            _req(t, name)
            if t.numel() < row * n:
                raise ValueError(f"{name} must hold n*{row} bytes")
    if not 0 <= log2_width <= 17:
        raise ValueError("log2_width must be 0..17")
    if (n << log2_width) >> 32:
        raise ValueError("n << log2_width must fit 32 bits")
    if validate and n:
        _check_merkle_layout(data, offsets, lens, log2w, log2_width, "hybrid_pieces")
        total = lens.to(torch.int64) + pads.to(torch.int64)
        if bool((pads.ne(0) & total.ne(16384 << log2_width)).any().item()) or bool(pads.lt(0).any().item()):
            raise ValueError("hybrid_pieces: a pad is neither 0 nor (16384 << log2_width) - len")
    sha1 = torch.empty((n, 20), dtype=torch.uint8, device=dev)
    roots = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    matched = torch.empty((n,), dtype=torch.uint8, device=dev) if (exp_sha1 is not None or
                                                                  exp_roots is not None) else None
    work = torch.empty((max(16, hybrid_work_bytes(n, log2_width)),), dtype=torch.uint8, device=dev)
    if stream is not None:  # the scratch outlives this call on the stream that uses it
        work.record_stream(stream)
    rc = lib().vx_hybrid_device_pieces(data.data_ptr(), offsets.data_ptr(), lens.data_ptr(), pads.data_ptr(),
                                       log2w.data_ptr() if log2w is not None else None, n, log2_width,
                                       work.data_ptr(), sha1.data_ptr(), roots.data_ptr(),
                                       exp_sha1.data_ptr() if exp_sha1 is not None else None,
                                       exp_roots.data_ptr() if exp_roots is not None else None,
                                       matched.data_ptr() if matched is not None else None,
                                       _stream_ptr(stream, dev))
    check(rc, "vx_hybrid_device_pieces")
    return sha1, roots, matched


def _zero_lens(lens, lo: int, hi: int, device, who: str) -> torch.Tensor:
    """The lengths of a zero-hash call as an int32 device tensor (the kernels
    read them as uint32): a host sequence of ints, checked here, or an int32
    device tensor, checked on the device with one copy back (a sync)."""
    if isinstance(lens, torch.Tensor):
        _req(lens, "lens", torch.int32)
        if lens.numel():
            mn, mx = torch.stack([lens.min(), lens.max()]).cpu().tolist()
            if mn < lo or mx > hi:
                raise ValueError(f"{who}: a length is outside {lo}..{hi}")
        return lens.reshape(-1)
    vals = [int(x) for x in lens]
    if any(not lo <= x <= hi for x in vals):
        raise ValueError(f"{who}: a length is outside {lo}..{hi}")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return torch.tensor(vals, dtype=torch.int64).to(torch.int32).to(dev)  # (above 2^31: the same bits)


def sha1_zeros(lens, device=None, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """SHA-1 of lens[j] zero bytes for every j, hashed from nothing
    (vx_sha1_device_zeros): the digest an unwritten piece's expected row is
    compared with when the re-verify skips file holes.  lens: a sequence of
    ints (0..2^32-1), or an int32 device tensor (0..2^31-1).  Returns [n,20]
    uint8 on the device.  Enqueue-only for a host sequence."""
    d_lens = _zero_lens(lens, 0, (1 << 32) - 1 if not isinstance(lens, torch.Tensor) else (1 << 31) - 1, device,
                        "sha1_zeros")
    n, dev = d_lens.numel(), d_lens.device
    out = torch.empty((n, 20), dtype=torch.uint8, device=dev)
    if stream is not None:
        d_lens.record_stream(stream)
        out.record_stream(stream)
    check(lib().vx_sha1_device_zeros(d_lens.data_ptr(), n, out.data_ptr(), _stream_ptr(stream, dev)),
          "vx_sha1_device_zeros")
    return out


def merkle_zero_leaves(lens, device=None, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """The v2 leaf rows of unwritten blocks (vx_merkle_device_zero_leaves):
    SHA-256 of lens[j] zero bytes, lens[j] in 1..16384, hashed from nothing.
    lens as for sha1_zeros.  Returns [n,32] uint8 on the device."""
    d_lens = _zero_lens(lens, 1, 16384, device, "merkle_zero_leaves")
    n, dev = d_lens.numel(), d_lens.device
    out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    if stream is not None:
        d_lens.record_stream(stream)
        out.record_stream(stream)
    check(lib().vx_merkle_device_zero_leaves(d_lens.data_ptr(), n, out.data_ptr(), _stream_ptr(stream, dev)),
          "vx_merkle_device_zero_leaves")
    return out


SKIP_ROW = 0xFFFFFFFF  # merkle_blocks: a block that stores no leaf row


def merkle_blocks(stage: torch.Tensor, rows: torch.Tensor, lens: torch.Tensor, leaves: torch.Tensor,
                  stream: Optional[torch.cuda.Stream] = None, validate: bool = True) -> torch.Tensor:
    """Hash 16 KiB stage blocks into leaf rows (vx_merkle_device_blocks): block
    b is stage[b*16384 : b*16384 + lens[b]] and its SHA-256 goes to row rows[b]
    of `leaves` ([R,32] uint8).  rows: int64 or int32 device tensor holding
    values 0..R-1 or SKIP_ROW (the block stores nothing); lens: int32, 0..16384;
    a block of length 0 stores the zero hash and is never read, so it may lie
    past the end of `stage`.  validate (default): rows in range, lengths in
    range and every read block inside `stage`, checked on the device with one
    copy back (a sync).  Returns `leaves`.  Enqueue-only otherwise."""
    _req(stage, "stage")
    _req(leaves, "leaves")
    _req(lens, "lens", torch.int32)
    if rows.dtype not in (torch.int64, torch.int32) or not rows.is_cuda or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous int64 or int32 device tensor")
    n = rows.numel()
    if lens.numel() != n:
        raise ValueError("rows and lens differ in length")
    dev = stage.device
    for name, t in (("rows", rows), ("lens", lens), ("leaves", leaves)):
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, stage on {dev}")
    if leaves.numel() % 32:
        raise ValueError("leaves must hold whole 32-byte rows")
    need64 = rows.dtype != torch.int32 or (validate and n)  # (an int32 table goes to the kernel as it is)
    r64 = rows.to(torch.int64) & 0xFFFFFFFF if need64 else None
    if validate and n:
        live = r64.ne(SKIP_ROW)
        read = live & lens.gt(0)
        ends = torch.arange(n, device=dev, dtype=torch.int64) * 16384 + lens.to(torch.int64)
        stats = torch.stack([
            torch.where(live, r64, torch.zeros_like(r64)).max(),
            lens.min().to(torch.int64),
            lens.max().to(torch.int64),
            torch.where(read, ends, torch.zeros_like(ends)).max(),
        ]).cpu().tolist()
        if stats[0] >= leaves.numel() // 32:
            raise ValueError(f"merkle_blocks: row {stats[0]} is outside leaves ({leaves.numel() // 32} rows)")
        if stats[1] < 0 or stats[2] > 16384:
            raise ValueError("merkle_blocks: a block length is outside 0..16384")
        if stats[3] > stage.numel():
            raise ValueError(f"merkle_blocks: a block ends at byte {stats[3]}, past the stage ({stage.numel()} bytes)")
    rows32 = r64.to(torch.int32) if rows.dtype != torch.int32 else rows  # (wraps SKIP_ROW to -1: the same bits)
    if stream is not None:
        rows32.record_stream(stream)
    rc = lib().vx_merkle_device_blocks(stage.data_ptr(), rows32.data_ptr(), lens.data_ptr(), n, leaves.data_ptr(),
                                       _stream_ptr(stream, dev))
    check(rc, "vx_merkle_device_blocks")
    return leaves


def merkle_nodes(leaves: torch.Tensor, n: int, log2_width: int, log2w: Optional[torch.Tensor] = None,
                 expected: Optional[torch.Tensor] = None, roots: Optional[torch.Tensor] = None,
                 matched: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None):
    """Reduce leaf rows already on the device to the roots of n pieces
    (vx_merkle_device_nodes): piece i's rows start at row i << log2_width and
    its tree has 2^log2w[i] slots (None: log2_width).  Returns (roots [n,32],
    matched [n] or None).  Enqueue-only."""
    _req(leaves, "leaves")
    dev = leaves.device
    if log2w is not None:
        _req(log2w, "log2w")
        if log2w.numel() != n or log2w.device != dev:
            raise ValueError("log2w must hold n widths on the leaves' device")
        if n and int(log2w.max()) > log2_width:
            raise ValueError("merkle_nodes: a log2w is above log2_width")
    leaves, roots, matched = _merkle_outputs(n, log2_width, dev, expected, leaves, roots, matched)
    rc = lib().vx_merkle_device_nodes(leaves.data_ptr(), log2w.data_ptr() if log2w is not None else None, n,
                                      log2_width, roots.data_ptr(),
                                      expected.data_ptr() if expected is not None else None,
                                      matched.data_ptr() if matched is not None else None,
                                      _stream_ptr(stream, dev))
    check(rc, "vx_merkle_device_nodes")
    return roots, matched


def merkle_leaf_check(window: torch.Tensor, row0: int, n: int, log2_width: int, leaf_first: torch.Tensor,
                      blocks: torch.Tensor, expected_leaves: Optional[torch.Tensor] = None,
                      bad: Optional[torch.Tensor] = None, wpp: Optional[int] = None,
                      shadow: Optional[torch.Tensor] = None, leaves_out: Optional[torch.Tensor] = None,
                      stream: Optional[torch.cuda.Stream] = None, validate: bool = True):
    """The leaf check of the files calls on its own (vx_merkle_device_leaf_check):
    n pieces whose leaf rows lie in `window` ([R,32] uint8), piece k's
    2^log2_width rows from row row0 + (k << log2_width) on; the first blocks[k]
    of them are live and stand for rows leaf_first[k].. of a compact leaf table
    (leaf_first, blocks: int32 [n]).

    expected_leaves ([T,32]): each live row is compared with its row of that
    table into `bad` (int64, the bitmap's uint64 words bit for bit; n * wpp
    words, wpp defaulting to max(1, 2^log2_width / 64); made zeroed if not
    given): block b of piece k is bit b & 63 of word k * wpp + (b >> 6); words
    above a piece's max(1, 2^log2_width / 64) stay as they were.  shadow (a
    tensor as large as window, needs expected_leaves): gets the table's rows at
    the window's rows, zeros at dead slots.  leaves_out ([T,32]): each live
    window row goes to its row of it.  Returns (bad, shadow, leaves_out).

    validate (default): 1 <= blocks[k] <= 2^log2_width and every table row
    inside expected_leaves / leaves_out, checked on the device with one copy
    back (a sync).  Enqueue-only otherwise."""
    _req(window, "window")
    _req(leaf_first, "leaf_first", torch.int32)
    _req(blocks, "blocks", torch.int32)
    if not 0 <= log2_width <= 17:
        raise ValueError("log2_width must be 0..17")
    if n < 0 or row0 < 0 or leaf_first.numel() != n or blocks.numel() != n:
        raise ValueError("leaf_first and blocks must hold n entries; n and row0 must be >= 0")
    rows = n << log2_width
    if (row0 + rows) >> 32:
        raise ValueError("row0 + (n << log2_width) must fit 32 bits")
    if window.numel() < 32 * (row0 + rows):
        raise ValueError("the pieces' rows end past the window")
    need = max(1, (1 << log2_width) // 64)
    wpp = need if wpp is None else wpp
    if wpp < need:
        raise ValueError("wpp must be at least max(1, 2^log2_width / 64)")
    if expected_leaves is None and leaves_out is None:
        raise ValueError("merkle_leaf_check: neither expected_leaves nor leaves_out asked for")
    if expected_leaves is None and (bad is not None or shadow is not None):
        raise ValueError("bad and shadow need expected_leaves")
    dev = window.device
    for name, t in (("leaf_first", leaf_first), ("blocks", blocks), ("expected_leaves", expected_leaves),
                    ("bad", bad), ("shadow", shadow), ("leaves_out", leaves_out)):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, window on {dev}")
    table_rows = None
    for name, t in (("expected_leaves", expected_leaves), ("leaves_out", leaves_out)):
        if t is not None:
            _req(t, name)
            if t.numel() % 32:
                raise ValueError(f"{name} must hold whole 32-byte rows")
            table_rows = t.numel() // 32 if table_rows is None else min(table_rows, t.numel() // 32)
    if expected_leaves is not None and leaves_out is not None and expected_leaves.data_ptr() == leaves_out.data_ptr():
        raise ValueError("leaves_out and expected_leaves must be different tensors")
    if expected_leaves is not None:
        if bad is None:
            bad = torch.zeros((n * wpp,), dtype=torch.int64, device=dev)
        else:
            _req(bad, "bad", torch.int64)
            if bad.numel() < n * wpp:
                raise ValueError("bad must hold n * wpp words")
    if shadow is not None:
        _req(shadow, "shadow")
        if shadow.numel() < 32 * (row0 + rows):
            raise ValueError("shadow must be as large as the window's rows in use")
    if validate and n:
        ends = leaf_first.to(torch.int64) + blocks.to(torch.int64)
        stats = torch.stack([blocks.min().to(torch.int64), blocks.max().to(torch.int64),
                             leaf_first.min().to(torch.int64), ends.max()]).cpu().tolist()
        if stats[0] < 1 or stats[1] > 1 << log2_width:
            raise ValueError("merkle_leaf_check: every blocks[k] must lie in 1..2^log2_width")
        if stats[2] < 0 or stats[3] > table_rows:
            raise ValueError(f"merkle_leaf_check: a piece's rows end at table row {stats[3]}, the table holds "
                             f"{table_rows}")
    rc = lib().vx_merkle_device_leaf_check(window.data_ptr(), row0, n, log2_width, wpp, leaf_first.data_ptr(),
                                           blocks.data_ptr(),
                                           expected_leaves.data_ptr() if expected_leaves is not None else None,
                                           bad.data_ptr() if bad is not None else None,
                                           shadow.data_ptr() if shadow is not None else None,
                                           leaves_out.data_ptr() if leaves_out is not None else None,
                                           _stream_ptr(stream, dev))
    check(rc, "vx_merkle_device_leaf_check")
    return bad, shadow, leaves_out


def merkle_root(layer: torch.Tensor, height: int = 0, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Root of a layer of hashes ([n,32] uint8) standing `height` levels above
    the leaves, padded to a power of two with pad hashes
    (vx_merkle_device_root).  Returns a [32] uint8 tensor.  Enqueue-only."""
    _req(layer, "layer")
    if layer.numel() == 0 or layer.numel() % 32:
        raise ValueError("layer must hold n >= 1 hashes of 32 bytes")
    n = layer.numel() // 32
    dev = layer.device
    work = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    root = torch.empty((32,), dtype=torch.uint8, device=dev)
    if stream is not None:  # the scratch outlives this call on the stream that uses it
        work.record_stream(stream)
    rc = lib().vx_merkle_device_root(layer.data_ptr(), n, height, work.data_ptr(), root.data_ptr(),
                                     _stream_ptr(stream, dev))
    check(rc, "vx_merkle_device_root")
    return root


def _upload(buf, dev, stream: Optional[torch.cuda.Stream]) -> torch.Tensor:
    """A host ctypes array as a uint8 device tensor, copied on the stream that
    will read it.  Through pinned memory and without blocking: a copy from
    pageable memory would wait for everything already on the stream, and the
    host's planning of one call could not overlap the kernels of the last
    (0.76 against 0.67 ms per call on one layer of 4 M hashes).
    torch keeps the pinned block alive until the copy has run."""
    host = torch.frombuffer(buf, dtype=torch.uint8).pin_memory()
    if stream is None:
        return host.to(dev, non_blocking=True)
    with torch.cuda.stream(stream):
        t = host.to(dev, non_blocking=True)
    return t


def merkle_layers(hashes: torch.Tensor, counts, height: int, expected: Optional[torch.Tensor] = None,
                  roots: Optional[torch.Tensor] = None, matched: Optional[torch.Tensor] = None,
                  stream: Optional[torch.cuda.Stream] = None):
    """Roots of many layers in one call (vx_merkle_device_layers): `hashes`
    ([sum(counts),32] uint8) holds the layers back to back, layer f counts[f]
    >= 1 hashes, all `height` levels above the leaves (a torrent's `piece
    layers`: merkle.layer_counts, height = log2(piece_length / 16 KiB)).
    counts is a host sequence: the host plans the tiles, the device runs one
    launch per pass (at most 4) whatever the number of layers.  With
    `expected` ([n,32], the files' `pieces root`) matched[f] = (root ==
    expected[f]).  roots: None allocates them, except with `expected` given,
    where None asks for verdicts only.  Returns (roots or None, matched or
    None).  Enqueue-only but for the upload of the tiles."""
    import ctypes

    from . import _lib

    _req(hashes, "hashes")
    dev = hashes.device
    n = len(counts)
    host_counts = [int(c) for c in counts]
    if any(not 0 <= c < 1 << 32 for c in host_counts):
        raise ValueError("merkle_layers: a count is outside 0..2^32-1")
    carr = (ctypes.c_uint32 * max(n, 1))(*host_counts)
    if not 0 <= height <= 64:
        raise ValueError("merkle_layers: height must be 0..64")
    plan = _lib.vx_merkle_layers_plan()
    check(lib().vx_merkle_layers_plan(carr, n, ctypes.byref(plan), None, 0), "vx_merkle_layers_plan")
    if hashes.numel() != 32 * plan.rows:
        raise ValueError(f"hashes must hold sum(counts) = {plan.rows} rows of 32 bytes")
    if roots is not None:
        _req(roots, "roots")
        if roots.numel() < 32 * n or roots.device != dev:
            raise ValueError("roots must hold n*32 bytes on the hashes' device")
    elif expected is None:
        roots = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    if expected is not None:
        _req(expected, "expected")
        if expected.numel() < 32 * n or expected.device != dev:
            raise ValueError("expected must hold n*32 bytes on the hashes' device")
        if matched is None:
            matched = torch.empty((n,), dtype=torch.uint8, device=dev)
        else:
            _req(matched, "matched")
            if matched.numel() < n or matched.device != dev:
                raise ValueError("matched must hold n bytes on the hashes' device")
    else:
        matched = None
    if n == 0:
        return roots, matched
    tiles = (_lib.vx_merkle_tile * plan.n_tiles)()
    check(lib().vx_merkle_layers_plan(carr, n, ctypes.byref(plan), tiles, plan.n_tiles), "vx_merkle_layers_plan")
    d_tiles = _upload(tiles, dev, stream)
    work = torch.empty((max(int(plan.work_rows), 1), 32), dtype=torch.uint8, device=dev)
    if stream is not None:  # the scratch and the tiles outlive this call on the stream that uses them
        work.record_stream(stream)
        d_tiles.record_stream(stream)
    rc = lib().vx_merkle_device_layers(hashes.data_ptr(), ctypes.byref(plan), d_tiles.data_ptr(), height,
                                       work.data_ptr(), roots.data_ptr() if roots is not None else None,
                                       expected.data_ptr() if expected is not None else None,
                                       matched.data_ptr() if matched is not None else None, _stream_ptr(stream, dev))
    check(rc, "vx_merkle_device_layers")
    return roots, matched


def merkle_trees(hashes: torch.Tensor, counts, height: int, tree: Optional[torch.Tensor] = None,
                 stream: Optional[torch.cuda.Stream] = None):
    """The trees of many layers in one call (vx_merkle_device_trees): `hashes`
    and `counts` as for :func:`merkle_layers`; every level of every layer's
    tree is kept (merkle.build_tree is the model), the trees back to back.
    Returns (tree, tree_off): tree is [sum(merkle.tree_rows(c)),32] uint8 on the
    hashes' device (None allocates it), tree_off a host list of n + 1 row
    offsets; the root of layer f is row tree_off[f + 1] - 1.  One launch per
    pass (at most 4).  Enqueue-only but for the upload of the tiles."""
    import ctypes

    from . import _lib

    _req(hashes, "hashes")
    dev = hashes.device
    n = len(counts)
    host_counts = [int(c) for c in counts]
    if any(not 0 <= c < 1 << 32 for c in host_counts):
        raise ValueError("merkle_trees: a count is outside 0..2^32-1")
    carr = (ctypes.c_uint32 * max(n, 1))(*host_counts)
    if not 0 <= height <= 64:
        raise ValueError("merkle_trees: height must be 0..64")
    plan = _lib.vx_merkle_tree_plan()
    off = (ctypes.c_uint64 * (n + 1))()
    check(lib().vx_merkle_tree_plan(carr, n, ctypes.byref(plan), None, 0, off), "vx_merkle_tree_plan")
    if hashes.numel() != 32 * plan.rows:
        raise ValueError(f"hashes must hold sum(counts) = {plan.rows} rows of 32 bytes")
    if tree is None:
        tree = torch.empty((int(plan.tree_rows), 32), dtype=torch.uint8, device=dev)
    else:
        _req(tree, "tree")
        if tree.numel() < 32 * plan.tree_rows or tree.device != dev:
            raise ValueError(f"tree must hold {plan.tree_rows} rows of 32 bytes on the hashes' device")
    if n == 0:
        return tree, list(off)
    tiles = (_lib.vx_merkle_tree_tile * plan.n_tiles)()
    check(lib().vx_merkle_tree_plan(carr, n, ctypes.byref(plan), tiles, plan.n_tiles, off), "vx_merkle_tree_plan")
    d_tiles = _upload(tiles, dev, stream)
    if stream is not None:  # the tiles outlive this call on the stream that uses them
        d_tiles.record_stream(stream)
    rc = lib().vx_merkle_device_trees(hashes.data_ptr(), ctypes.byref(plan), d_tiles.data_ptr(), height,
                                      tree.data_ptr(), _stream_ptr(stream, dev))
    check(rc, "vx_merkle_device_trees")
    return tree, list(off)


def check_proofs(proofs, n_rows: int, n_expected: int):
    """A host sequence of proofs, each (pos, row, expected, span, uncles) or a
    ``vx_merkle_proof``, as a ctypes array after the checks of
    vx_merkle_verify_proofs: span a power of two of at most 512, uncles <= 64,
    row + span + uncles <= n_rows, expected < n_expected.  ValueError names the
    first bad index."""
    from . import _lib

    arr = _lib.proof_array(proofs)
    for i in range(len(proofs)):
        span, uncles = arr[i].span, arr[i].uncles
        if not (1 <= span <= _lib.VX_MERKLE_TILE_ROWS and span & (span - 1) == 0):
            raise ValueError(f"proof {i}: span is not a power of two in 1..512")
        if uncles > 64:
            raise ValueError(f"proof {i}: uncles > 64")
        if arr[i].row + span + uncles > n_rows:
            raise ValueError(f"proof {i}: row + span + uncles > n_rows")
        if arr[i].expected >= n_expected:
            raise ValueError(f"proof {i}: expected >= n_expected")
    return arr


def merkle_proofs(hashes: torch.Tensor, proofs, expected: torch.Tensor,
                  stream: Optional[torch.cuda.Stream] = None):
    """Verify hash proofs in one call of two launches
    (vx_merkle_device_proofs).  `hashes` ([R,32] uint8) holds every proof's
    rows as they came off the wire, its span then its uncles; `proofs` is a
    host sequence of (pos, row, expected, span, uncles) (or
    ``vx_merkle_proof``), checked as by :func:`check_proofs`; `expected`
    ([E,32]) the trusted rows.  Returns (tops [n,32], matched [n]): tops[i] is
    where proof i's walk ended, matched[i] = (tops[i] == expected[proofs[i].expected]).
    Enqueue-only but for the upload of the proofs."""
    _req(hashes, "hashes")
    _req(expected, "expected")
    dev = hashes.device
    if expected.device != dev:
        raise ValueError(f"expected is on {expected.device}, hashes on {dev}")
    if hashes.numel() % 32 or expected.numel() % 32:
        raise ValueError("hashes and expected must hold whole 32-byte rows")
    n = len(proofs)
    arr = check_proofs(proofs, hashes.numel() // 32, expected.numel() // 32)
    tops = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    matched = torch.empty((n,), dtype=torch.uint8, device=dev)
    if n == 0:
        return tops, matched
    d_proofs = _upload(arr, dev, stream)
    if stream is not None:
        d_proofs.record_stream(stream)
    rc = lib().vx_merkle_device_proofs(hashes.data_ptr(), d_proofs.data_ptr(), n, tops.data_ptr(),
                                       expected.data_ptr(), matched.data_ptr(), _stream_ptr(stream, dev))
    check(rc, "vx_merkle_device_proofs")
    return tops, matched


def ragged_plan(lens_host) -> tuple[int, int]:
    """(longest piece, total bytes) of a ragged batch: the `plan` argument of
    :func:`sha1_ragged`."""
    import numpy as np

    arr = np.asarray(lens_host, dtype=np.uint64)
    return (int(arr.max()) if arr.size else 0), int(arr.sum())


def length_order(lens_host) -> torch.Tensor:
    """Permutation sorting pieces by descending length (vx_sort_order), as
    an int32 CPU tensor; move it to the device for sha1_ragged."""
    import ctypes

    import numpy as np

    arr = np.ascontiguousarray(np.asarray(lens_host, dtype=np.uint32))
    out = np.empty_like(arr)
    check(lib().vx_sort_order(arr.ctypes.data, arr.size, out.ctypes.data), "vx_sort_order")
    del ctypes
    return torch.from_numpy(out.astype(np.int32))


def synth_fill(data: torch.Tensor, n: int, piece_len: int, stride: Optional[int] = None, first: int = 0,
               seed: int = 0x5EED0002, corrupt_every: int = 0,
               stream: Optional[torch.cuda.Stream] = None) -> None:
    """Fill n synthetic pieces on the device (DESIGN.md "Synthetic pieces";
    include/vx_synth.h, a test/bench generator: tuning build only)."""
    _req(data, "data")
    stride = piece_len if stride is None else stride
    if n > 0 and (n - 1) * stride + piece_len > data.numel():
        raise ValueError("batch exceeds data tensor")
    rc = tuning().vx_synth_fill(data.data_ptr(), stride, piece_len, n, first, seed, corrupt_every,
                                _stream_ptr(stream, data.device))
    check(rc, "vx_synth_fill", tuning())
