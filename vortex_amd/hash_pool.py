"""Host-side mirror of vortex's hashing-pool boundary, backed by the HIP engine.

The reference has no trait for this path; its "interface" is three call sites
(SURVEY.md §8b), mirrored here under the reference's own names:

===============================  ==============================================
reference                        here
===============================  ==============================================
``scope.spawn(hash closure)``    :meth:`HashPool.spawn`
  peer_connection.rs:1139-1158     (index, conn_id, buffer, piece_len, expected)
``downloaded_piece_rc.try_recv`` :meth:`HashPool.try_recv` → ``DownloadedPiece``
  torrent.rs:415-442
``DownloadedPiece``              :class:`DownloadedPiece` (piece_selector.rs:311-317)
``par_iter().map(check).collect``:func:`verify_pieces` → ``list[bool]``
  torrent.rs:724-740
===============================  ==============================================

A BitTorrent v2 (BEP 52) piece takes the same path under
:meth:`HashPool.spawn_merkle` / :meth:`HashPool.try_recv_merkle`: its result is
the piece's SHA-256 merkle root (vx_merkle_submit / vx_merkle_poll).  A piece
of a hybrid (v1 + v2) torrent takes it once for both hashes under
:meth:`HashPool.spawn_hybrid` / :meth:`HashPool.try_recv_hybrid`
(vx_hybrid_submit / vx_hybrid_poll → :class:`DownloadedHybridPiece`).

Semantics kept from the reference:
* a hash mismatch is a value (``hash_matched=False``), never an exception;
* the buffer is moved into the job and handed back in ``DownloadedPiece``
  (the caller must return it to its pool, buf_pool.rs:21-30);
* the digest covers exactly ``buffer[:piece_len]`` (peer_connection.rs:1148) —
  pool buffers are reused without zeroing, bytes past piece_len are ignored;
* completions arrive in batch-completion order, not submission order.

All hashing runs in libvortex_amd.so on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Any, Optional, Sequence

from . import _lib, merkle
from ._lib import CONFIG_OPTIONS, VxError, check, lib, proof_array, vx_completion, vx_config, vx_stats


@dataclass
class DownloadedPiece:
    """piece_selector.rs:311-317."""

    index: int
    conn_id: int
    hash_matched: bool
    buffer: Any
    digest: bytes = b""


@dataclass
class DownloadedHybridPiece:
    """A hybrid (v1 + v2) piece's result (vx_hybrid_poll): ``matched`` has bit 0
    set when the SHA-1 was given and equal and bit 1 when the root was."""

    index: int
    conn_id: int
    matched: int
    buffer: Any
    sha1: bytes = b""
    root: bytes = b""

    @property
    def hash_matched(self) -> bool:
        return self.matched == 3


@dataclass
class BlockVerdicts:
    """What HashPool.verify_merkle_files_blocks returns for a range of pieces;
    unpacks as (matched, layer_ok, bad, bad_counts)."""

    matched: list
    layer_ok: list
    bad: list  # the bitmap's uint64 words, len(bad) / len(matched) per piece
    bad_counts: list
    io_errors: int = 0

    def __iter__(self):
        return iter((self.matched, self.layer_ok, self.bad, self.bad_counts))

    def blocks(self, i: int) -> list:
        """The set blocks of piece i of the range, in order."""
        wpp = len(self.bad) // max(1, len(self.matched))
        return [64 * k + b for k in range(wpp) for b in range(64) if self.bad[i * wpp + k] >> b & 1]


def _addr_of(buf) -> tuple[int, Any]:
    """Stable address of a writable or read-only buffer plus a keep-alive."""
    if isinstance(buf, (bytes,)):
        keep = ctypes.create_string_buffer(buf, len(buf))
        return ctypes.addressof(keep), keep
    try:
        import numpy as np

        if isinstance(buf, np.ndarray):
            return buf.ctypes.data, buf
    except ImportError:  # pragma: no cover
        pass
    mv = memoryview(buf)
    if mv.readonly:
        keep = ctypes.create_string_buffer(mv.tobytes(), mv.nbytes)
        return ctypes.addressof(keep), keep
    c = (ctypes.c_uint8 * mv.nbytes).from_buffer(mv)
    return ctypes.addressof(c), (c, mv)


class HashPool:
    """The GPU engine behind vortex's spawn / try_recv hash boundary.

    ``piece_length`` is the torrent's piece_length (the BufferPool buffer
    size, torrent.rs:344).  One HashPool per torrent, used from one thread.
    ``options`` set the other vx_config fields (include/vx_hash.h, ABI 2):
    zero_copy, direct_io, batch_chunk, verify_chunk, verify_cold_chunk,
    verify_ramp; unset ones keep vx_config_default's values (each must fit
    the field's uint32: negative or >= 2**32 values are refused here, ctypes
    would wrap them silently).  ``hooks=True`` creates the context in the
    test build libvortex_amd_tuning.so, for fault injection
    (include/vx_tuning.h); ``self.lib`` is the library holding the context.
    """

    def __init__(self, piece_length: int, device: int = 0, slots: Optional[int] = None,
                 batch_pieces: Optional[int] = None, slot_bytes: Optional[int] = None, hooks: bool = False,
                 **options):
        L = _lib.tuning() if hooks else lib()
        self.lib = L
        cfg = vx_config()
        L.vx_config_default(ctypes.byref(cfg), piece_length)
        cfg.device = device
        if slots is not None:
            cfg.slots = slots
        if slot_bytes is not None:
            cfg.slot_bytes = slot_bytes
        if batch_pieces is not None:
            cfg.batch_pieces = batch_pieces
        for name, value in options.items():
            if name not in CONFIG_OPTIONS:
                raise TypeError(f"HashPool: unknown option {name!r} (vx_config has {', '.join(CONFIG_OPTIONS)})")
            if not 0 <= int(value) < 1 << 32:
                raise ValueError(f"HashPool: option {name}={value} outside the uint32 range of vx_config")
            setattr(cfg, name, int(value))
        h = ctypes.c_void_p()
        check(L.vx_create(ctypes.byref(cfg), ctypes.byref(h)), "vx_create", L)
        self._h = h
        self.config = cfg
        self._next_tag = 0
        self._inflight: dict[int, tuple[int, int, Any, Any]] = {}
        self._cbuf = (vx_completion * 1024)()
        self._cbuf_v2 = (_lib.vx_merkle_completion * 1024)()
        self._cbuf_hy = (_lib.vx_hybrid_completion * 1024)()
        self._registered: dict[int, tuple[int, Any, Any]] = {}  # id(buf) -> (address, keep-alive, buf)
        self._hybrid_rows = 0  # rows of the tables given to set_hybrid_tables
        self._skip_holes = False  # vx_set_skip_holes' default
        self._merkle_zero_copy = False  # vx_set_merkle_zero_copy's default

    # -- lifecycle ---------------------------------------------------------
    def close(self) -> None:
        if self._h:
            check(self.lib.vx_destroy(self._h), "vx_destroy", self.lib)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    # -- buffer pinning (buf_pool.rs / buf_ring.rs AnonymousMmap) -----------
    def register_buffer(self, buf) -> None:
        """Pin a pool buffer (an mmap, bytearray or numpy array) for direct
        DMA.  Read-only objects such as ``bytes`` are refused: pinning them
        would pin a private copy that no later piece points into.  The
        registration is keyed by the object, so ``unregister_buffer`` must be
        given the same object."""
        mv = memoryview(buf)
        if mv.readonly:
            raise ValueError("register_buffer needs a writable buffer (e.g. an mmap or bytearray), not a read-only one")
        if id(buf) in self._registered:
            raise ValueError("buffer is already registered with this pool")
        addr, keep = _addr_of(buf)
        check(self.lib.vx_register_host_buffer(self._h, addr, mv.nbytes), "vx_register_host_buffer", self.lib)
        self._registered[id(buf)] = (addr, keep, buf)

    def unregister_buffer(self, buf) -> None:
        ent = self._registered.get(id(buf))
        if ent is None or ent[2] is not buf:
            raise ValueError("buffer was not registered with this pool")
        check(self.lib.vx_unregister_host_buffer(self._h, ent[0]), "vx_unregister_host_buffer", self.lib)
        del self._registered[id(buf)]

    # -- download path -------------------------------------------------------
    def spawn(self, index: int, conn_id: int, buffer, piece_len: int, expected_hash: Optional[bytes] = None) -> None:
        """peer_connection.rs:1145-1158: hash buffer[:piece_len] against
        expected_hash (or, when None, against row `index` of the table given
        to set_piece_table); the result comes back from try_recv().

        Ownership (include/vx_hash.h): the piece is taken iff the submit
        returns 0.  Otherwise this raises VxError whose ``refused`` is
        ``(index, conn_id, buffer)``: the piece was not taken, no result will
        ever carry it, it is not in take_unfinished(), and the caller hashes
        it on its own pool.  On VX_EDEVICE the pool is dead: collect the rest
        with try_iter() until it raises, then take_unfinished()."""
        if expected_hash is not None and len(expected_hash) != 20:
            raise ValueError("expected_hash must be 20 bytes")
        addr, keep = _addr_of(buffer)
        if piece_len > memoryview(buffer).nbytes:
            raise ValueError("piece_len exceeds buffer size")
        tag = self._next_tag
        self._next_tag += 1
        if expected_hash is None:
            rc, where = self.lib.vx_submit_piece(self._h, tag, addr, piece_len, index), "vx_submit_piece"
        else:
            exp = ctypes.create_string_buffer(bytes(expected_hash), 20)
            rc, where = self.lib.vx_submit(self._h, tag, addr, piece_len, exp), "vx_submit"
        if rc != 0:
            try:
                check(rc, where, self.lib)
            except VxError as e:
                e.refused = (index, conn_id, buffer)
                raise
        self._inflight[tag] = (index, conn_id, buffer, keep)

    def spawn_merkle(self, index: int, conn_id: int, buffer, piece_len: int,
                     expected_root: Optional[bytes] = None, log2w: Optional[int] = None) -> None:
        """spawn() for a BitTorrent v2 (BEP 52) piece (vx_merkle_submit): the
        SHA-256 merkle root of buffer[:piece_len] over 16 KiB blocks, as a
        tree of 2^log2w leaf slots (default: piece_length / 16 KiB, the width
        of every piece of a file longer than piece_length; merkle.file_pieces
        gives the width of a short file's single piece), compared with
        expected_root (32 bytes; None: the root is only returned).  The result
        comes back from try_recv_merkle() / try_iter_merkle(), never from
        try_recv().  Ownership and errors as for spawn()."""
        if expected_root is not None and len(expected_root) != 32:
            raise ValueError("expected_root must be 32 bytes")
        if log2w is None:
            log2w = max(0, (int(self.config.max_piece_len) // _lib.VX_MERKLE_BLOCK).bit_length() - 1)
        if not 0 <= int(log2w) < 1 << 32:
            raise ValueError("log2w outside the uint32 range")
        addr, keep = _addr_of(buffer)
        if piece_len > memoryview(buffer).nbytes:
            raise ValueError("piece_len exceeds buffer size")
        tag = self._next_tag
        self._next_tag += 1
        exp = ctypes.create_string_buffer(bytes(expected_root), 32) if expected_root is not None else None
        rc = self.lib.vx_merkle_submit(self._h, tag, addr, piece_len, int(log2w), exp)
        if rc != 0:
            try:
                check(rc, "vx_merkle_submit", self.lib)
            except VxError as e:
                e.refused = (index, conn_id, buffer)
                raise
        self._inflight[tag] = (index, conn_id, buffer, keep)

    def spawn_hybrid(self, index: int, conn_id: int, buffer, piece_len: int, pad_len: int = 0,
                     expected_sha1: Optional[bytes] = None, expected_root: Optional[bytes] = None,
                     log2w: Optional[int] = None) -> None:
        """spawn() for a piece of a hybrid (v1 + v2) torrent (vx_hybrid_submit):
        one submit, one transfer and one result carry both hashes.  The SHA-1
        is over buffer[:piece_len] followed by pad_len zeros that exist nowhere
        (the BEP 47 pad behind a file's last piece, hybrid.hybrid_pieces), the
        merkle root over buffer[:piece_len] alone as a tree of 2^log2w leaf
        slots (default as spawn_merkle).  With both expected values None the
        piece is compared with row `index` of the tables given to
        set_hybrid_tables (vx_hybrid_submit_piece), or, when no tables are
        set, with nothing: the hashes are only returned.  With one given, only
        that side is compared.  The result comes back from try_recv_hybrid() /
        try_iter_hybrid() only.  Ownership and errors as for spawn()."""
        if expected_sha1 is not None and len(expected_sha1) != 20:
            raise ValueError("expected_sha1 must be 20 bytes")
        if expected_root is not None and len(expected_root) != 32:
            raise ValueError("expected_root must be 32 bytes")
        if log2w is None:
            log2w = max(0, (int(self.config.max_piece_len) // _lib.VX_MERKLE_BLOCK).bit_length() - 1)
        for name, value in (("piece_len", piece_len), ("pad_len", pad_len), ("log2w", log2w)):
            if not 0 <= int(value) < 1 << 32:
                raise ValueError(f"{name} outside the uint32 range")
        by_index = expected_sha1 is None and expected_root is None and self._hybrid_rows > 0
        if by_index and not 0 <= int(index) < 1 << 32:
            raise ValueError("index outside the uint32 range")
        if piece_len > memoryview(buffer).nbytes:
            raise ValueError("piece_len exceeds buffer size")
        addr, keep = _addr_of(buffer)
        tag = self._next_tag
        self._next_tag += 1
        if by_index:
            rc, where = self.lib.vx_hybrid_submit_piece(self._h, tag, addr, piece_len, int(pad_len), int(log2w),
                                                        int(index)), "vx_hybrid_submit_piece"
        else:
            e1 = ctypes.create_string_buffer(bytes(expected_sha1), 20) if expected_sha1 is not None else None
            e2 = ctypes.create_string_buffer(bytes(expected_root), 32) if expected_root is not None else None
            rc, where = self.lib.vx_hybrid_submit(self._h, tag, addr, piece_len, int(pad_len), int(log2w), e1,
                                                  e2), "vx_hybrid_submit"
        if rc != 0:
            try:
                check(rc, where, self.lib)
            except VxError as e:
                e.refused = (index, conn_id, buffer)
                raise
        self._inflight[tag] = (index, conn_id, buffer, keep)

    def set_hybrid_tables(self, pieces: bytes, roots: bytes) -> None:
        """Upload a hybrid torrent's v1 `pieces` string (n x 20 B) and its v2
        rows (n x 32 B, numbered as hybrid.hybrid_pieces numbers the pieces)
        once (vx_hybrid_set_piece_tables); afterwards spawn_hybrid with no
        expected values compares on the device by index.  Independent of
        set_piece_table; needs nothing pending."""
        if len(pieces) % 20 or len(roots) % 32 or len(pieces) // 20 != len(roots) // 32:
            raise ValueError("pieces holds 20 bytes and roots 32 bytes per piece")
        n = len(roots) // 32
        if n >= 1 << 32:
            raise ValueError("more than 2^32 - 1 pieces")
        b1 = ctypes.create_string_buffer(bytes(pieces), max(1, len(pieces)))
        b2 = ctypes.create_string_buffer(bytes(roots), max(1, len(roots)))
        check(self.lib.vx_hybrid_set_piece_tables(self._h, b1, b2, n), "vx_hybrid_set_piece_tables", self.lib)
        self._hybrid_rows = n

    def set_piece_table(self, pieces: bytes) -> None:
        """Upload the torrent's `pieces` string (n x 20 B) once; afterwards
        spawn(..., expected_hash=None) compares on the device by index."""
        if len(pieces) % 20:
            raise ValueError("pieces table must be a multiple of 20 bytes")
        buf = ctypes.create_string_buffer(bytes(pieces), max(1, len(pieces)))
        check(self.lib.vx_set_piece_table(self._h, buf, len(pieces) // 20), "vx_set_piece_table", self.lib)

    def flush(self) -> None:
        """Launch everything queued; call once per event-loop turn."""
        check(self.lib.vx_flush(self._h), "vx_flush", self.lib)

    def _poll(self, max_items: int) -> list[DownloadedPiece]:
        k = check(self.lib.vx_poll(self._h, self._cbuf, min(max_items, len(self._cbuf))), "vx_poll", self.lib)
        out = []
        for j in range(k):
            r = self._cbuf[j]
            index, conn_id, buffer, _keep = self._inflight.pop(r.tag)
            out.append(DownloadedPiece(index, conn_id, bool(r.matched), buffer, bytes(r.digest)))
        return out

    def try_recv(self) -> Optional[DownloadedPiece]:
        """torrent.rs:418 `downloaded_piece_rc.try_recv()`: non-blocking."""
        got = self._poll(1)
        return got[0] if got else None

    def try_iter(self) -> list[DownloadedPiece]:
        """Everything completed so far (the `while let Ok(..) = try_recv()` loop)."""
        out = []
        while True:
            try:
                got = self._poll(len(self._cbuf))
            except VxError:
                if out:  # hand out what was already taken off the engine; the error is sticky
                    return out  # and the next call raises it
                raise
            out.extend(got)
            if len(got) < len(self._cbuf):
                return out

    def _poll_merkle(self, max_items: int) -> list[DownloadedPiece]:
        k = check(self.lib.vx_merkle_poll(self._h, self._cbuf_v2, min(max_items, len(self._cbuf_v2))),
                  "vx_merkle_poll", self.lib)
        out = []
        for j in range(k):
            r = self._cbuf_v2[j]
            index, conn_id, buffer, _keep = self._inflight.pop(r.tag)
            out.append(DownloadedPiece(index, conn_id, bool(r.matched), buffer, bytes(r.root)))
        return out

    def try_recv_merkle(self) -> Optional[DownloadedPiece]:
        """try_recv() for v2 pieces (vx_merkle_poll): `digest` is the 32-byte
        merkle root.  Pieces given to spawn() never arrive here."""
        got = self._poll_merkle(1)
        return got[0] if got else None

    def try_iter_merkle(self) -> list[DownloadedPiece]:
        """Every v2 piece completed so far (try_iter() for spawn_merkle)."""
        out = []
        while True:
            try:
                got = self._poll_merkle(len(self._cbuf_v2))
            except VxError:
                if out:  # as try_iter: the error is sticky and the next call raises it
                    return out
                raise
            out.extend(got)
            if len(got) < len(self._cbuf_v2):
                return out

    def _poll_hybrid(self, max_items: int) -> list[DownloadedHybridPiece]:
        k = check(self.lib.vx_hybrid_poll(self._h, self._cbuf_hy, min(max_items, len(self._cbuf_hy))),
                  "vx_hybrid_poll", self.lib)
        out = []
        for j in range(k):
            r = self._cbuf_hy[j]
            index, conn_id, buffer, _keep = self._inflight.pop(r.tag)
            out.append(DownloadedHybridPiece(index, conn_id, int(r.matched), buffer, bytes(r.sha1), bytes(r.root)))
        return out

    def try_recv_hybrid(self) -> Optional[DownloadedHybridPiece]:
        """try_recv() for hybrid pieces (vx_hybrid_poll).  Pieces given to
        spawn() or spawn_merkle() never arrive here."""
        got = self._poll_hybrid(1)
        return got[0] if got else None

    def try_iter_hybrid(self) -> list[DownloadedHybridPiece]:
        """Every hybrid piece completed so far (try_iter() for spawn_hybrid)."""
        out = []
        while True:
            try:
                got = self._poll_hybrid(len(self._cbuf_hy))
            except VxError:
                if out:  # as try_iter: the error is sticky and the next call raises it
                    return out
                raise
            out.extend(got)
            if len(got) < len(self._cbuf_hy):
                return out

    def take_unfinished(self) -> list[tuple[int, int, Any]]:
        """After a device error (a VxError from spawn / try_recv / try_iter, or
        their _merkle and _hybrid forms; pieces of all three kinds are listed):
        (index, conn_id, buffer) of every TAKEN piece whose result never came
        back, for the caller to hash on its own pool (INTEGRATION.md "Device
        failure").  A spawn that raised did not take its piece (it is in the
        exception's ``refused``), so it is not listed here.  Close the pool
        before reusing those buffers: that waits for the device to stop
        reading them."""
        out = [(index, conn_id, buffer) for index, conn_id, buffer, _keep in self._inflight.values()]
        self._inflight.clear()
        return out

    def drain(self, timeout_ms: int = 0) -> None:
        """Flush and wait for all in-flight pieces (the scope join of
        event_loop.rs:385-602); results stay queued for try_recv."""
        check(self.lib.vx_drain(self._h, timeout_ms), "vx_drain", self.lib)

    @property
    def pending(self) -> int:
        return int(self.lib.vx_pending(self._h))

    # -- observability (vx_get_stats) -------------------------------------------
    def stats(self) -> dict:
        """The engine's counters (include/vx_hash.h vx_stats) as a dict; the
        latency histogram is a list of VX_STATS_HIST log2 buckets in us."""
        st = vx_stats()
        check(self.lib.vx_get_stats(self._h, ctypes.byref(st)), "vx_get_stats", self.lib)
        out = {name: int(getattr(st, name)) for name, _ in vx_stats._fields_ if name != "batch_latency_hist"}
        out["batch_latency_hist"] = [int(x) for x in st.batch_latency_hist]
        return out

    def reset_stats(self) -> None:
        check(self.lib.vx_reset_stats(self._h), "vx_reset_stats", self.lib)

    def last_verify(self) -> dict:
        """Where the last verify_files call spent its time (vx_hash.h
        vx_last_verify), plus the derived rates bench.py records: the
        readers' pread rate, the data copies' GPU-timed rate, and the fraction
        of the copy span the copy engine was busy."""
        t = _lib.vx_verify_trace()
        check(self.lib.vx_last_verify(self._h, ctypes.byref(t)), "vx_last_verify", self.lib)
        d = {name: getattr(t, name) for name, _ in _lib.vx_verify_trace._fields_}
        gib = float(1 << 30)
        d["read_GiBps_per_thread"] = t.read_bytes / gib / (t.read_busy_ms * 1e-3) if t.read_busy_ms else None
        d["read_GiBps"] = t.read_bytes / gib / (t.read_span_ms * 1e-3) if t.read_span_ms else None
        d["copy_GiBps"] = t.copy_bytes / gib / (t.copy_busy_ms * 1e-3) if t.copy_busy_ms else None
        d["copy_busy_frac"] = t.copy_busy_ms / t.copy_span_ms if t.copy_span_ms else None
        return d

    @property
    def skip_holes(self) -> bool:
        """Whether verify_files / verify_merkle_files / verify_hybrid_files
        judge ranges the file system never wrote without reading them
        (vx_set_skip_holes): whole pieces (v1), 16 KiB blocks
        (v2), 256 KiB chunks (hybrid).  Off by default; the split and the hash
        calls ignore it."""
        return self._skip_holes

    @skip_holes.setter
    def skip_holes(self, on: bool) -> None:
        check(self.lib.vx_set_skip_holes(self._h, 1 if on else 0), "vx_set_skip_holes", self.lib)
        self._skip_holes = bool(on)

    def last_verify_holes(self) -> dict:
        """What the last verify_files / verify_merkle_files /
        verify_hybrid_files call skipped (vx_last_verify_holes): hole_pieces
        (no byte read), hole_blocks (16 KiB blocks not read; the hybrid call
        counts those of its hole pieces too), hole_bytes, the extents scanned,
        scan_ms and zero_hash_ms.  All zero with skip_holes off."""
        t = _lib.vx_hole_trace()
        check(self.lib.vx_last_verify_holes(self._h, ctypes.byref(t)), "vx_last_verify_holes", self.lib)
        return {name: getattr(t, name) for name, _ in _lib.vx_hole_trace._fields_}

    @property
    def merkle_zero_copy(self) -> bool:
        """Whether spawn_merkle's slots of registered, 16-byte aligned pieces
        are hashed straight out of host memory (vx_set_merkle_zero_copy,
        DESIGN.md §6.5).  Off by default; read when a slot is launched, so it
        may change while pieces are pending.  Results and stats() are the same
        either way; merkle_zero_copy_trace() says what it did."""
        return self._merkle_zero_copy

    @merkle_zero_copy.setter
    def merkle_zero_copy(self, on: bool) -> None:
        check(self.lib.vx_set_merkle_zero_copy(self._h, 1 if on else 0), "vx_set_merkle_zero_copy", self.lib)
        self._merkle_zero_copy = bool(on)

    def merkle_zero_copy_trace(self) -> dict:
        """Since the pool was made (vx_merkle_zero_copy_trace): v2 slots
        launched zero-copy, their pieces and bytes, and fallback_slots, the v2
        slots that took the gathered path while the setting was on."""
        t = _lib.merkle_zc_trace_type()()
        check(self.lib.vx_merkle_zero_copy_trace(self._h, ctypes.byref(t)), "vx_merkle_zero_copy_trace", self.lib)
        return {name: getattr(t, name) for name in _lib.MERKLE_ZC_TRACE_FIELDS}

    def last_verify_rounds(self) -> list[dict]:
        """The last verify_files call's round timeline (vx_last_verify_rounds):
        per chunk round, ms from the call's start — reads queued / done, copy
        enqueued, the GPU's copy start / end and kernel end — with its bytes,
        chunk offset, lanes and VX_ROUND_* flags.  Empty on the whole-piece
        path."""
        n = check(self.lib.vx_last_verify_rounds(self._h, None, 0), "vx_last_verify_rounds", self.lib)
        arr = (_lib.vx_verify_round * max(1, n))()
        n = check(self.lib.vx_last_verify_rounds(self._h, arr, n), "vx_last_verify_rounds", self.lib)
        return [{name: getattr(arr[k], name) for name, _ in _lib.vx_verify_round._fields_} for k in range(n)]

    # -- bulk verify -----------------------------------------------------------
    def sha1_batch(self, pieces: Sequence) -> list[bytes]:
        n = len(pieces)
        ptrs, lens, keep = _ptr_arrays(pieces)
        out = ctypes.create_string_buffer(20 * max(n, 1))
        check(self.lib.vx_sha1_batch(self._h, ptrs, lens, n, out), "vx_sha1_batch", self.lib)
        raw = out.raw
        return [raw[20 * i: 20 * i + 20] for i in range(n)]

    def verify_files(self, paths: Sequence[str], file_lengths: Sequence[int], piece_length: int,
                     expected: bytes, io_threads: int = 0, first: int = 0,
                     count: int | None = None) -> tuple[list[bool], int]:
        """State::from_metadata_and_root's bulk re-verify (torrent.rs:716-761):
        pieces read from the torrent's files (file_store.rs:228-303 byte
        ranges) and verified on the GPU.  Returns (verdicts, pieces with I/O
        errors).  `expected` is the torrent's `pieces` string (n*20 bytes).
        first/count restrict it to pieces [first, first+count) (one rank's
        shard, vx_verify_files_range); the verdicts then cover that range."""
        return _verify_files(self, paths, file_lengths, piece_length, expected, io_threads, first, count)

    def verify_files_split(self, paths: Sequence[str], file_lengths: Sequence[int], piece_length: int,
                           expected: bytes, split: "Split", io_threads: int = 0) -> int:
        """The engine's side of a split re-verify (vx_verify_files_split):
        verifies the pieces it claims from `split` while the caller's pool
        claims the others, writes their verdicts into split.matched and
        returns how many of its pieces hit an I/O error.  Blocks; run the pool
        on other threads (ctypes drops the GIL for the call)."""
        arr = (ctypes.c_char_p * max(1, len(paths)))(*[os.fsencode(p) for p in paths])
        lens = (ctypes.c_uint64 * max(1, len(file_lengths)))(*file_lengths)
        exp = ctypes.create_string_buffer(bytes(expected), max(1, len(expected)))
        rc = self.lib.vx_verify_files_split(self._h, arr, lens, len(paths), piece_length, exp, len(expected) // 20,
                                            ctypes.byref(split.s), split.matched, io_threads)
        return int(check(rc, "vx_verify_files_split", self.lib))

    def verify_batch(self, pieces: Sequence, expected: Sequence[bytes]) -> tuple[list[bool], list[bytes]]:
        n = len(pieces)
        if len(expected) != n:
            raise ValueError("expected must have one digest per piece")
        ptrs, lens, keep = _ptr_arrays(pieces)
        exp = ctypes.create_string_buffer(b"".join(bytes(e) for e in expected), 20 * max(n, 1))
        matched = ctypes.create_string_buffer(max(n, 1))
        dig = ctypes.create_string_buffer(20 * max(n, 1))
        check(self.lib.vx_verify_batch(self._h, ptrs, lens, exp, n, matched, dig), "vx_verify_batch", self.lib)
        raw = dig.raw
        return [bool(b) for b in matched.raw[:n]], [raw[20 * i: 20 * i + 20] for i in range(n)]

    def verify_merkle(self, pieces: Sequence, expected: Sequence[bytes], piece_length: int,
                      log2w: Optional[Sequence[int]] = None) -> tuple[list[bool], list[bytes]]:
        """BitTorrent v2 (BEP 52) bulk verify (vx_merkle_verify_batch): piece i
        against expected[i], the 32-byte root of its SHA-256 merkle tree over
        16 KiB blocks (a `piece layers` entry; for a file of at most
        piece_length bytes its `pieces root`, with log2w[i] from
        merkle.file_pieces).  Returns (verdicts, roots)."""
        n = len(pieces)
        if len(expected) != n or (log2w is not None and len(log2w) != n):
            raise ValueError("expected (and log2w) must have one entry per piece")
        ptrs, lens, keep = _ptr_arrays(pieces)
        exp = ctypes.create_string_buffer(b"".join(bytes(e) for e in expected), 32 * max(n, 1))
        lw = (ctypes.c_uint8 * max(n, 1))(*log2w) if log2w is not None else None
        matched = ctypes.create_string_buffer(max(n, 1))
        roots = ctypes.create_string_buffer(32 * max(n, 1))
        check(self.lib.vx_merkle_verify_batch(self._h, ptrs, lens, lw, n, piece_length, exp, matched, roots),
              "vx_merkle_verify_batch", self.lib)
        raw = roots.raw
        return [bool(b) for b in matched.raw[:n]], [raw[32 * i: 32 * i + 32] for i in range(n)]

    def verify_piece_layers(self, layers: Sequence[bytes], roots: Sequence[bytes], piece_length: int) -> list[bool]:
        """Check a v2 torrent's `piece layers` against the files' `pieces root`
        (vx_merkle_verify_layers): layers[f] is one file's string of 32-byte
        piece hashes, roots[f] that file's `pieces root`; every layer is padded
        to a power of two with the pad hash of a piece and reduced on the
        device, all files in one call.  Only after this may the layers serve as
        the `expected` of the piece calls.  Works while async pieces are
        pending and leaves stats() alone.  Returns one bool per file."""
        n = len(layers)
        if len(roots) != n:
            raise ValueError("roots must have one `pieces root` per layer")
        if any(len(x) == 0 or len(x) % 32 for x in layers) or any(len(r) != 32 for r in roots):
            raise ValueError("a layer is a non-empty string of 32-byte hashes, a root 32 bytes")
        height = merkle.log2_width(piece_length)
        blob = b"".join(bytes(x) for x in layers)
        hashes = ctypes.create_string_buffer(blob, max(1, len(blob)))
        counts = (ctypes.c_uint32 * max(n, 1))(*[len(x) // 32 for x in layers])
        exp = ctypes.create_string_buffer(b"".join(bytes(r) for r in roots), 32 * max(n, 1))
        out = ctypes.create_string_buffer(max(n, 1))
        check(self.lib.vx_merkle_verify_layers(self._h, hashes, counts, n, height, exp, out, None),
              "vx_merkle_verify_layers", self.lib)
        return [bool(b) for b in out.raw[:n]]

    def verify_hash_proofs(self, hashes: bytes, proofs: Sequence, expected: Sequence[bytes]) -> list[bool]:
        """Verify BEP 52 `hashes` messages in one call
        (vx_merkle_verify_proofs): `hashes` holds every proof's rows as they
        came off the wire (its span, then its uncles), proofs[i] =
        (pos, row, expected, span, uncles) says where proof i's rows start,
        which span of its layer it is and which of the trusted rows in
        `expected` its walk must reach.  The engine checks every number first
        (VxError VX_EINVAL names the first bad proof).  Works while async
        pieces are pending and leaves stats() alone.  Returns one bool per
        proof."""
        n = len(proofs)
        if len(hashes) % 32 or any(len(e) != 32 for e in expected):
            raise ValueError("hashes and expected hold whole 32-byte rows")
        arr = proof_array(proofs)
        buf = ctypes.create_string_buffer(bytes(hashes), max(1, len(hashes)))
        exp = ctypes.create_string_buffer(b"".join(bytes(e) for e in expected), 32 * max(len(expected), 1))
        out = ctypes.create_string_buffer(max(n, 1))
        check(self.lib.vx_merkle_verify_proofs(self._h, buf, len(hashes) // 32, arr, n, exp, len(expected), out,
                                               None), "vx_merkle_verify_proofs", self.lib)
        return [bool(b) for b in out.raw[:n]]

    def check_blocks(self, pieces: Sequence, piece_length: int, expected_leaves: Optional[Sequence[bytes]] = None,
                     want_leaves: bool = False) -> tuple[Optional[list[list[int]]], Optional[list[bytes]]]:
        """Which 16 KiB blocks of v2 pieces are wrong (vx_merkle_check_blocks):
        expected_leaves[i] is piece i's leaf layer, piece_length / 16 KiB rows
        of 32 bytes, as a peer sent it for a `hashes` request at base layer 0
        and verify_hash_proofs accepted it against the piece's trusted row.
        Every piece is a tree of piece_length / 16 KiB slots.  Works while
        async pieces are pending and leaves stats() alone.

        Returns (bad, leaves): bad[i] the indices of piece i's bad blocks, in
        order (None without expected_leaves; a slot at or past the piece's end
        is never bad); leaves[i] the piece's own leaf layer
        (merkle.leaf_rows), what a seeder answers such a request from (None
        unless want_leaves)."""
        n = len(pieces)
        lw = merkle.log2_width(piece_length)
        rows = 1 << lw
        if expected_leaves is None and not want_leaves:
            raise ValueError("check_blocks: neither expected_leaves nor want_leaves")
        if expected_leaves is not None and (len(expected_leaves) != n or
                                            any(len(e) != 32 * rows for e in expected_leaves)):
            raise ValueError("expected_leaves must hold piece_length / 16 KiB rows of 32 bytes per piece")
        ptrs, lens, keep = _ptr_arrays(pieces)
        wpp = max(1, rows // 64)
        exp = bad = counts = out = None
        if expected_leaves is not None:
            exp = ctypes.create_string_buffer(b"".join(bytes(e) for e in expected_leaves), 32 * rows * max(n, 1))
            bad = (ctypes.c_uint64 * max(n * wpp, 1))()
            counts = (ctypes.c_uint32 * max(n, 1))()
        if want_leaves:
            out = ctypes.create_string_buffer(32 * rows * max(n, 1))
        check(self.lib.vx_merkle_check_blocks(self._h, ptrs, lens, n, piece_length, exp, bad, counts, out),
              "vx_merkle_check_blocks", self.lib)
        lists = None
        if bad is not None:
            lists = [[64 * k + b for k in range(wpp) for b in range(64) if bad[i * wpp + k] >> b & 1]
                     if counts[i] else [] for i in range(n)]
        leaves = None
        if out is not None:
            view = memoryview(out)
            leaves = [bytes(view[32 * rows * i:32 * rows * (i + 1)]) for i in range(n)]
        return lists, leaves

    def verify_merkle_files(self, paths: Sequence[str], file_lengths: Sequence[int], piece_length: int,
                            expected: bytes, io_threads: int = 0, first: int = 0,
                            count: int | None = None) -> tuple[list[bool], int]:
        """BitTorrent v2 (BEP 52) re-verify from disk (vx_merkle_verify_files):
        the pieces of every file, numbered file by file
        (merkle.torrent_pieces), read in rounds of 16 KiB blocks and verified
        against `expected` (n*32 bytes: each file's `piece layers` entry, or
        its `pieces root` for a file of at most piece_length bytes).  The
        piece length is not bounded by the pool's.  Returns (verdicts, pieces
        with I/O errors); first/count restrict the call to pieces
        [first, first+count) and the verdicts then cover that range."""
        n = len(expected) // 32
        if count is None:
            count = n - first
        arr = (ctypes.c_char_p * max(1, len(paths)))(*[os.fsencode(p) for p in paths])
        lens = (ctypes.c_uint64 * max(1, len(file_lengths)))(*file_lengths)
        exp = ctypes.create_string_buffer(bytes(expected), max(1, len(expected)))
        out = ctypes.create_string_buffer(max(1, count))
        if first == 0 and count == n:
            rc = self.lib.vx_merkle_verify_files(self._h, arr, lens, len(paths), piece_length, exp, n, out,
                                                 io_threads)
        else:
            rc = self.lib.vx_merkle_verify_files_range(self._h, arr, lens, len(paths), piece_length, exp, n, first,
                                                       count, out, io_threads)
        bad = check(rc, "vx_merkle_verify_files", self.lib)
        return [bool(b) for b in out.raw[:count]], int(bad)

    def verify_hybrid_files(self, paths: Sequence[str], file_lengths: Sequence[int], piece_length: int,
                            pieces: bytes, roots: bytes, first: int = 0, count: int | None = None,
                            io_threads: int = 0) -> list[tuple[bool, bool]]:
        """Re-verify a hybrid (v1 + v2, BEP 52 "upgrade path") torrent from
        disk in one pass (vx_hybrid_verify_files): `paths` / `file_lengths`
        list the real files only, the BEP 47 pad files between them are
        implied and never read; `pieces` is the v1 `pieces` table (n*20
        bytes), `roots` what verify_merkle_files takes (n*32 bytes), pieces
        numbered as hybrid.hybrid_pieces numbers them.  Every byte is read and
        copied to the device once and feeds both hashes; with skip_holes, 256
        KiB chunks the file system never wrote are not read at all.  Returns one
        (v1_ok, v2_ok) per piece of [first, first+count); a piece that could
        not be read is (False, False) and counts in stats()["io_errors"]."""
        n = len(roots) // 32
        if len(pieces) != 20 * n or len(roots) != 32 * n:
            raise ValueError("pieces holds 20 bytes and roots 32 bytes per piece")
        if count is None:
            count = n - first
        arr = (ctypes.c_char_p * max(1, len(paths)))(*[os.fsencode(p) for p in paths])
        lens = (ctypes.c_uint64 * max(1, len(file_lengths)))(*file_lengths)
        exp1 = ctypes.create_string_buffer(bytes(pieces), max(1, len(pieces)))
        exp2 = ctypes.create_string_buffer(bytes(roots), max(1, len(roots)))
        out = ctypes.create_string_buffer(max(1, count))
        if first == 0 and count == n:
            rc = self.lib.vx_hybrid_verify_files(self._h, arr, lens, len(paths), piece_length, exp1, exp2, n, out,
                                                 io_threads)
        else:
            rc = self.lib.vx_hybrid_verify_files_range(self._h, arr, lens, len(paths), piece_length, exp1, exp2, n,
                                                       first, count, out, io_threads)
        check(rc, "vx_hybrid_verify_files", self.lib)
        return [(bool(b & 1), bool(b & 2)) for b in out.raw[:count]]

    # ---- creating a torrent: the tables the verify calls take, made from the files ----

    def hash_files(self, paths: Sequence[str], file_lengths: Sequence[int], piece_length: int, io_threads: int = 0,
                   first: int = 0, count: int | None = None) -> tuple[bytes, list[bool], int]:
        """A v1 torrent's `pieces` string from its files (vx_hash_files): the
        layout of verify_files, the SHA-1 of every piece.  Returns (digests,
        ok, pieces with I/O errors): count * 20 bytes, and ok[i] False (its
        digest all zero) where a byte of the piece could not be read.
        first/count restrict the call to pieces [first, first+count)."""
        n = (sum(file_lengths) + piece_length - 1) // piece_length if piece_length > 0 else 0
        if count is None:
            count = n - first
        arr, lens = _path_arrays(paths, file_lengths)
        dig = ctypes.create_string_buffer(20 * max(1, count))
        ok = ctypes.create_string_buffer(max(1, count))
        if first == 0 and count == n:
            rc = self.lib.vx_hash_files(self._h, arr, lens, len(paths), piece_length, n, dig, ok, io_threads)
        else:
            rc = self.lib.vx_hash_files_range(self._h, arr, lens, len(paths), piece_length, n, first, count, dig, ok,
                                              io_threads)
        bad = check(rc, "vx_hash_files", self.lib)
        return dig.raw[:20 * count], [bool(b) for b in ok.raw[:count]], int(bad)

    def hash_merkle_files(self, paths: Sequence[str], file_lengths: Sequence[int], piece_length: int,
                          io_threads: int = 0, first: int = 0, count: int | None = None,
                          trees: bool = True) -> tuple[bytes, list[bool], Optional[bytes], int]:
        """A v2 torrent's hashes from its files (vx_merkle_hash_files).
        Returns (rows, ok, tree, pieces with I/O errors): rows is what
        verify_merkle_files takes as `expected` (32 bytes per piece); tree
        holds every non-empty file's layer tree, laid out by
        merkle.tree_layout: the last row of a file's tree is its `pieces
        root`, its first rows are its `piece layers` entry, and the levels
        between answer hash requests (merkle.proof_from_tree).  A piece that
        could not be read has ok False and a zero row, and its file a zero
        tree.  A range call (first/count) or trees=False returns tree None."""
        n = len(merkle.torrent_pieces(file_lengths, piece_length)[0])
        if count is None:
            count = n - first
        arr, lens = _path_arrays(paths, file_lengths)
        rows = ctypes.create_string_buffer(32 * max(1, count))
        ok = ctypes.create_string_buffer(max(1, count))
        tree = None
        if first == 0 and count == n:
            tree_rows = merkle.tree_layout(file_lengths, piece_length)[1][-1] if trees else 0
            tree = ctypes.create_string_buffer(32 * max(1, tree_rows)) if trees else None
            rc = self.lib.vx_merkle_hash_files(self._h, arr, lens, len(paths), piece_length, n, rows, ok, tree,
                                               tree_rows, io_threads)
        else:
            rc = self.lib.vx_merkle_hash_files_range(self._h, arr, lens, len(paths), piece_length, n, first, count,
                                                     rows, ok, io_threads)
        bad = check(rc, "vx_merkle_hash_files", self.lib)
        return (rows.raw[:32 * count], [bool(b) for b in ok.raw[:count]],
                tree.raw[:32 * tree_rows] if tree is not None else None, int(bad))

    def hash_merkle_files_leaves(self, paths: Sequence[str], file_lengths: Sequence[int], piece_length: int,
                                 io_threads: int = 0, first: int = 0, count: int | None = None,
                                 trees: bool = True) -> tuple[bytes, list[bool], Optional[bytes], int, bytes]:
        """hash_merkle_files that also keeps the 16 KiB leaf layer
        (vx_merkle_hash_files_leaves), in the same pass.  Returns (rows, ok,
        tree, pieces with I/O errors, leaves): the first four as
        hash_merkle_files; leaves is the torrent's leaf table, laid out by
        merkle.leaf_layout (merkle.file_leaf_table is its model): what a seeder
        answers `hashes` requests at base layer 0 from and what
        verify_merkle_files_blocks takes.  A piece that could not be read has
        zero leaf rows.  A range call (first/count) returns the rows of its
        pieces only: rows [leaf_first[first], leaf_first[first + count - 1] +
        blocks[first + count - 1]) of the table."""
        leaf_first, blocks, leaf_rows = merkle.leaf_layout(file_lengths, piece_length)
        n = len(leaf_first)
        if count is None:
            count = n - first
        arr, lens = _path_arrays(paths, file_lengths)
        rows = ctypes.create_string_buffer(32 * max(1, count))
        ok = ctypes.create_string_buffer(max(1, count))
        leaves = ctypes.create_string_buffer(32 * max(1, leaf_rows))
        tree = None
        if first == 0 and count == n:
            tree_rows = merkle.tree_layout(file_lengths, piece_length)[1][-1] if trees else 0
            tree = ctypes.create_string_buffer(32 * max(1, tree_rows)) if trees else None
            rc = self.lib.vx_merkle_hash_files_leaves(self._h, arr, lens, len(paths), piece_length, n, rows, ok, tree,
                                                      tree_rows, leaves, leaf_rows, io_threads)
        else:
            rc = self.lib.vx_merkle_hash_files_leaves_range(self._h, arr, lens, len(paths), piece_length, n, first,
                                                            count, rows, ok, leaves, leaf_rows, io_threads)
        bad = check(rc, "vx_merkle_hash_files_leaves", self.lib)
        lo, hi = (leaf_first[first], leaf_first[first + count - 1] + blocks[first + count - 1]) if count else (0, 0)
        return (rows.raw[:32 * count], [bool(b) for b in ok.raw[:count]],
                tree.raw[:32 * tree_rows] if tree is not None else None, int(bad), leaves.raw[32 * lo:32 * hi])

    def verify_merkle_files_blocks(self, paths: Sequence[str], file_lengths: Sequence[int], piece_length: int,
                                   expected: bytes, leaves: bytes, first: int | None = None,
                                   count: int | None = None, io_threads: int = 0) -> "BlockVerdicts":
        """verify_merkle_files that also says which 16 KiB blocks are wrong, in
        the same single pass (vx_merkle_verify_files_blocks).  `leaves` is the
        torrent's stored leaf table (hash_merkle_files_leaves, or a client's
        resume data; merkle.leaf_layout).  Returns BlockVerdicts(matched,
        layer_ok, bad, bad_counts, io_errors) over pieces [first, first +
        count): matched as verify_merkle_files; layer_ok[i] whether the stored
        leaf rows of piece i reduce to its expected row (it does not depend on
        the data); bad the bitmap's uint64 words, merkle.bitmap_words(count,
        log2_width(piece_length)) of them, block b of piece i being bit b & 63
        of word i * wpp + (b >> 6) (BlockVerdicts.blocks(i) lists them);
        bad_counts[i] the set bits of piece i.

        matched: the data is good, and set bits can only name stale stored
        rows (layer_ok is then False).  Not matched and layer_ok: the set bits
        are exactly the blocks to fetch again.  Neither: fetch the piece, or
        its leaf layer first.  A piece that lacks bytes has every existing
        block set."""
        n = len(expected) // 32
        first = 0 if first is None else first
        if count is None:
            count = n - first
        lw = merkle.log2_width(piece_length)
        if len(leaves) % 32:
            raise ValueError("leaves must hold whole 32-byte rows")
        arr, lens = _path_arrays(paths, file_lengths)
        exp = ctypes.create_string_buffer(bytes(expected), max(1, len(expected)))
        tab = ctypes.create_string_buffer(bytes(leaves), max(1, len(leaves)))
        words = merkle.bitmap_words(max(count, 0), lw)
        out = ctypes.create_string_buffer(max(1, count))
        layer = ctypes.create_string_buffer(max(1, count))
        bad = (ctypes.c_uint64 * max(1, words))()
        counts = (ctypes.c_uint32 * max(1, count))()
        if first == 0 and count == n:
            rc = self.lib.vx_merkle_verify_files_blocks(self._h, arr, lens, len(paths), piece_length, exp, n, tab,
                                                        len(leaves) // 32, out, layer, bad, counts, io_threads)
        else:
            rc = self.lib.vx_merkle_verify_files_blocks_range(self._h, arr, lens, len(paths), piece_length, exp, n,
                                                              tab, len(leaves) // 32, first, count, out, layer, bad,
                                                              counts, io_threads)
        errs = check(rc, "vx_merkle_verify_files_blocks", self.lib)
        return BlockVerdicts([bool(b) for b in out.raw[:count]], [bool(b) for b in layer.raw[:count]],
                             list(bad[:words]), list(counts[:count]), int(errs))

    def hash_hybrid_files(self, paths: Sequence[str], file_lengths: Sequence[int], piece_length: int,
                          io_threads: int = 0, first: int = 0, count: int | None = None,
                          trees: bool = True) -> tuple[bytes, bytes, list[bool], Optional[bytes], int]:
        """A hybrid torrent's hashes from its files in one pass
        (vx_hybrid_hash_files): (pieces, rows, ok, tree, pieces with I/O
        errors).  `pieces` is the v1 table over data plus implied pad zeros, as
        verify_hybrid_files takes it; rows, ok and tree as hash_merkle_files."""
        n = len(merkle.torrent_pieces(file_lengths, piece_length)[0])
        if count is None:
            count = n - first
        arr, lens = _path_arrays(paths, file_lengths)
        sha1 = ctypes.create_string_buffer(20 * max(1, count))
        rows = ctypes.create_string_buffer(32 * max(1, count))
        ok = ctypes.create_string_buffer(max(1, count))
        tree = None
        if first == 0 and count == n:
            tree_rows = merkle.tree_layout(file_lengths, piece_length)[1][-1] if trees else 0
            tree = ctypes.create_string_buffer(32 * max(1, tree_rows)) if trees else None
            rc = self.lib.vx_hybrid_hash_files(self._h, arr, lens, len(paths), piece_length, n, sha1, rows, ok, tree,
                                               tree_rows, io_threads)
        else:
            rc = self.lib.vx_hybrid_hash_files_range(self._h, arr, lens, len(paths), piece_length, n, first, count,
                                                     sha1, rows, ok, io_threads)
        bad = check(rc, "vx_hybrid_hash_files", self.lib)
        return (sha1.raw[:20 * count], rows.raw[:32 * count], [bool(b) for b in ok.raw[:count]],
                tree.raw[:32 * tree_rows] if tree is not None else None, int(bad))

    def build_piece_trees(self, layers: Sequence[bytes], piece_length: int) -> tuple[list[bytes], list[bytes]]:
        """The trees of a v2 torrent's `piece layers` (vx_merkle_build_trees),
        for a client that has the layers from a .torrent and starts seeding:
        layers[f] is one file's string of 32-byte piece hashes.  Returns
        (trees, roots): trees[f] is merkle.build_tree(layers[f], height) with
        height = log2(piece_length / 16 KiB), roots[f] its last row.  Works
        while async pieces are pending and leaves stats() alone."""
        n = len(layers)
        if any(len(x) == 0 or len(x) % 32 for x in layers):
            raise ValueError("a layer is a non-empty string of 32-byte hashes")
        height = merkle.log2_width(piece_length)
        blob = b"".join(bytes(x) for x in layers)
        hashes = ctypes.create_string_buffer(blob, max(1, len(blob)))
        counts = [len(x) // 32 for x in layers]
        carr = (ctypes.c_uint32 * max(n, 1))(*counts)
        off = [0]
        for c in counts:
            off.append(off[-1] + merkle.tree_rows(c))
        tree = ctypes.create_string_buffer(32 * max(1, off[-1]))
        roots = ctypes.create_string_buffer(32 * max(1, n))
        check(self.lib.vx_merkle_build_trees(self._h, hashes, carr, n, height, tree, roots),
              "vx_merkle_build_trees", self.lib)
        view, raw = memoryview(tree), roots.raw
        return ([bytes(view[32 * off[f]:32 * off[f + 1]]) for f in range(n)],
                [raw[32 * f:32 * f + 32] for f in range(n)])


def _path_arrays(paths: Sequence[str], file_lengths: Sequence[int]):
    """A files call's paths and lengths as ctypes arrays."""
    arr = (ctypes.c_char_p * max(1, len(paths)))(*[os.fsencode(p) for p in paths])
    lens = (ctypes.c_uint64 * max(1, len(file_lengths)))(*file_lengths)
    return arr, lens


def _verify_files(pool: "HashPool", paths: Sequence[str], file_lengths: Sequence[int], piece_length: int,
                  expected: bytes, io_threads: int = 0, first: int = 0,
                  count: int | None = None) -> tuple[list[bool], int]:
    n = len(expected) // 20
    if count is None:
        count = n - first
    arr = (ctypes.c_char_p * max(1, len(paths)))(*[os.fsencode(p) for p in paths])
    lens = (ctypes.c_uint64 * max(1, len(file_lengths)))(*file_lengths)
    exp = ctypes.create_string_buffer(bytes(expected), max(1, len(expected)))
    out = ctypes.create_string_buffer(max(1, count))
    if first == 0 and count == n:
        rc = pool.lib.vx_verify_files(pool._h, arr, lens, len(paths), piece_length, exp, n, out, io_threads)
    else:
        rc = pool.lib.vx_verify_files_range(pool._h, arr, lens, len(paths), piece_length, exp, n, first, count, out,
                                         io_threads)
    bad = check(rc, "vx_verify_files", pool.lib)
    return [bool(b) for b in out.raw[:count]], int(bad)


class Split:
    """One bulk re-verify shared at once by the engine and the caller's pool,
    with no plan (include/vx_hash.h vx_split / vx_verify_files_split): the
    pool's threads take pieces from the head with claim() and report each
    finished one with done(); the engine (HashPool.verify_files_split) takes
    groups from the top, sized from both sides' rates measured as it goes.
    `matched` holds every verdict once both sides have returned: entries
    [0, boundary - first) are the pool's to write, the rest the engines'.
    claim_fn / done_fn / arg are the C addresses a native pool calls."""

    def __init__(self, first: int, end: int, cpu_threads: int = 0, cpu_thread_rate: float = 0.0):
        self._bind(_lib.vx_split(), ctypes.create_string_buffer(max(1, end - first)), first, end)
        self._init(cpu_threads, cpu_thread_rate, 1)

    @classmethod
    def attach(cls, buf, first: int, end: int, init: bool, cpu_threads: int = 0, cpu_thread_rate: float = 0.0,
               engines: int = 1) -> "Split":
        """A split living in a shared buffer (e.g. a MAP_SHARED mmap of a
        /dev/shm file, one per node): the vx_split at offset 0, the end - first
        verdict bytes after it, so engines in several processes (one per GPU)
        and the pool claim from one word and write one verdict array.  One
        process inits (init=True) before the others attach."""
        self = cls.__new__(cls)
        self._bind(_lib.vx_split.from_buffer(buf, 0),
                   (ctypes.c_char * max(1, end - first)).from_buffer(buf, ctypes.sizeof(_lib.vx_split)), first, end)
        if init:
            self._init(cpu_threads, cpu_thread_rate, engines)
        return self

    def _bind(self, s, matched, first: int, end: int) -> None:
        self.lib = lib()
        self.s, self.matched = s, matched
        self.first, self.end = first, end
        self.arg = ctypes.addressof(self.s)
        self.claim_fn = ctypes.cast(self.lib.vx_split_claim, ctypes.c_void_p).value
        self.done_fn = ctypes.cast(self.lib.vx_split_done, ctypes.c_void_p).value

    def _init(self, cpu_threads: int, cpu_thread_rate: float, engines: int) -> None:
        check(self.lib.vx_split_init(ctypes.byref(self.s), self.first, self.end, cpu_threads, cpu_thread_rate),
              "vx_split_init", self.lib)
        self.s.engines = engines

    def claim(self) -> int:
        """The next piece for the pool, or -1 when none is left."""
        return int(self.lib.vx_split_claim(ctypes.byref(self.s)))

    def done(self, pieces: int = 1) -> None:
        self.lib.vx_split_done(ctypes.byref(self.s), pieces)

    @property
    def boundary(self) -> int:
        """The engine's lowest piece (end when it took none)."""
        return int(self.lib.vx_split_boundary(ctypes.byref(self.s)))

    @property
    def pool_done(self) -> int:
        return int(self.s.pool_done)

    def verdicts(self) -> list[bool]:
        return [bool(b) for b in bytes(self.matched)[:self.end - self.first]]


def verify_files_multi(pools: Sequence["HashPool"], paths: Sequence[str], file_lengths: Sequence[int],
                       piece_length: int, expected: bytes, io_threads: int = 0) -> tuple[list[bool], int]:
    """In-process multi-GPU re-verify (vx_verify_files_multi): one HashPool
    per GPU (or several on one), pieces split into contiguous ranges across
    them, each range verified on its own host thread.  Same result as
    HashPool.verify_files on one pool: (verdicts, pieces with I/O errors)."""
    if not pools:
        raise ValueError("need at least one pool")
    L = pools[0].lib
    if any(p.lib is not L for p in pools):
        raise ValueError("verify_files_multi: every pool must come from the same library (hooks)")
    n = len(expected) // 20
    ctxs = (ctypes.c_void_p * len(pools))(*[p._h.value for p in pools])
    arr = (ctypes.c_char_p * max(1, len(paths)))(*[os.fsencode(p) for p in paths])
    lens = (ctypes.c_uint64 * max(1, len(file_lengths)))(*file_lengths)
    exp = ctypes.create_string_buffer(bytes(expected), max(1, len(expected)))
    out = ctypes.create_string_buffer(max(1, n))
    rc = L.vx_verify_files_multi(ctxs, len(pools), arr, lens, len(paths), piece_length, exp, n, out, io_threads)
    bad = check(rc, "vx_verify_files_multi", L)
    return [bool(b) for b in out.raw[:n]], int(bad)


def verify_files_split_multi(pools: Sequence["HashPool"], paths: Sequence[str], file_lengths: Sequence[int],
                             piece_length: int, expected: bytes, split: "Split", io_threads: int = 0) -> int:
    """The split over several GPUs (vx_verify_files_split_multi): every pool
    is one engine claiming from `split` on its own host thread, beside the
    caller's pool on split.claim().  Verdicts land in split.matched; returns
    the engines' pieces with I/O errors.  Blocks; run the pool on other
    threads."""
    if not pools:
        raise ValueError("need at least one pool")
    L = pools[0].lib
    if any(p.lib is not L for p in pools):
        raise ValueError("verify_files_split_multi: every pool must come from the same library (hooks)")
    ctxs = (ctypes.c_void_p * len(pools))(*[p._h.value for p in pools])
    arr = (ctypes.c_char_p * max(1, len(paths)))(*[os.fsencode(p) for p in paths])
    lens = (ctypes.c_uint64 * max(1, len(file_lengths)))(*file_lengths)
    exp = ctypes.create_string_buffer(bytes(expected), max(1, len(expected)))
    rc = L.vx_verify_files_split_multi(ctxs, len(pools), arr, lens, len(paths), piece_length, exp,
                                       len(expected) // 20, ctypes.byref(split.s), split.matched, io_threads)
    return int(check(rc, "vx_verify_files_split_multi", L))


def _ptr_arrays(pieces: Sequence):
    n = len(pieces)
    keep = []
    ptrs = (ctypes.c_void_p * max(n, 1))()
    lens = (ctypes.c_uint32 * max(n, 1))()
    for i, p in enumerate(pieces):
        addr, k = _addr_of(p if len(p) else b"\0")
        keep.append(k)
        ptrs[i] = addr
        lens[i] = len(p)
    return ptrs, lens, keep


def verify_pieces(pieces: Sequence, expected: Sequence[bytes], device: int = 0,
                  piece_length: Optional[int] = None) -> list[bool]:
    """torrent.rs:724-740: one verdict per piece, in piece order."""
    plen = piece_length or max((len(p) for p in pieces), default=1) or 1
    with HashPool(plen, device=device) as pool:
        matched, _ = pool.verify_batch(pieces, expected)
    return matched


def piece_len(index: int, num_pieces: int, piece_length: int, total_length: int) -> int:
    """PieceSelector::piece_len with the last-piece rule (piece_selector.rs:63-69, 291-298)."""
    last = total_length % piece_length or piece_length
    return last if index == num_pieces - 1 else piece_length


__all__ = ["DownloadedPiece", "DownloadedHybridPiece", "HashPool", "verify_pieces", "verify_files_multi", "piece_len", "plan_verify",
           "plan_verify_split"]


def plan_verify(n_pieces: int, piece_length: int, total_length: int, cpu_threads: int = 0,
                cpu_thread_rate: float = 0.0, n_gpus: int = 1) -> dict:
    """Where a bulk verify should run (include/vx_hash.h vx_plan_verify_gpus,
    host-only, no GPU): the predicted seconds of the GPU path over n_gpus
    contexts and of the caller's pool of cpu_threads (torrent.rs:724-740), and
    use_gpu.  0 threads / rate = 16 threads at 2.2e9 B/s (SHA-NI)."""
    p = _lib.vx_plan()
    check(lib().vx_plan_verify_gpus(n_pieces, piece_length, total_length, cpu_threads, cpu_thread_rate, n_gpus,
                                    ctypes.byref(p)), "vx_plan_verify_gpus")
    out = {name: getattr(p, name) for name, _ in _lib.vx_plan._fields_ if not name.startswith("_")}
    out["use_gpu"] = bool(out["use_gpu"])
    return out


def plan_verify_split(n_pieces: int, piece_length: int, total_length: int, cpu_threads: int = 0,
                      cpu_thread_rate: float = 0.0, n_gpus: int = 1) -> dict:
    """Split one bulk verify between the GPUs and the caller's own pool run
    at once (include/vx_hash.h vx_plan_verify_split, host-only): the GPUs take
    pieces [gpu_first, n_pieces), the pool the rest; the plan's predicted
    times for both sides.  gpu_count 0 = keep the pool alone."""
    p = _lib.vx_plan()
    first, count = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib().vx_plan_verify_split(n_pieces, piece_length, total_length, cpu_threads, cpu_thread_rate, n_gpus,
                                     ctypes.byref(first), ctypes.byref(count), ctypes.byref(p)),
          "vx_plan_verify_split")
    out = {name: getattr(p, name) for name, _ in _lib.vx_plan._fields_ if not name.startswith("_")}
    out["use_gpu"] = bool(out["use_gpu"])
    out["gpu_first"], out["gpu_count"] = int(first.value), int(count.value)
    return out
