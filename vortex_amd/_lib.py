"""ctypes binding of libvortex_amd.so (the C ABI declared in include/vx_hash.h).

The library is the product: there is no CPU or PyTorch fallback.  If it is
missing, loading raises ``ImportError`` (fail loudly, never silently degrade).

``lib()`` is the release library vortex links (vx_hash.h only).  ``tuning()``
is libvortex_amd_tuning.so, the same sources built with the test hooks: it
also exports include/vx_tuning.h (kernel-variant pins, fault injection, clock
stamps) and include/vx_synth.h (the synthetic-piece generator) for tests and
bench.py.  A context lives in the library that created it: pass a handle
only to functions of that same library (HashPool(hooks=True) creates its
context in tuning()).

``torch`` is imported before the library is loaded on purpose: torch ships its
own ``libamdhip64.so`` (same soname ``libamdhip64.so.7``) and loading it first
makes our library bind to that single HIP runtime instead of pulling in a
second one from /opt/rocm.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvortex_amd.so")
TUNING_PATH = os.path.join(_HERE, "libvortex_amd_tuning.so")

VX_OK = 0
VX_EINVAL = -22
VX_ENOMEM = -12
VX_ERANGE = -34
VX_ENODEV = -19
VX_EDEVICE = -5
VX_EBUSY = -16

VX_MERKLE_BLOCK = 16384  # BitTorrent v2 (BEP 52) leaf block
VX_SHA256_LEN = 32

# Every function include/vx_hash.h declares: what libvortex_amd.so exports,
# and all it exports (tests/test_abi.py checks the headers and both libraries'
# dynamic symbols against these lists).
EXPORTS = (
    "vx_abi_version", "vx_last_error", "vx_strerror", "vx_device_count", "vx_config_default",
    "vx_create", "vx_destroy", "vx_register_host_buffer", "vx_unregister_host_buffer",
    "vx_submit", "vx_flush", "vx_poll", "vx_drain", "vx_pending", "vx_set_piece_table", "vx_submit_piece",
    "vx_sha1_batch", "vx_verify_batch", "vx_verify_files", "vx_verify_files_range", "vx_verify_files_multi",
    "vx_sha1_device_uniform", "vx_sha1_device_ragged", "vx_sha1_device_ragged_hint", "vx_sort_order",
    "vx_plan_verify", "vx_plan_verify_gpus", "vx_plan_verify_split", "vx_get_stats", "vx_reset_stats",
    "vx_last_verify", "vx_last_verify_rounds",
    "vx_split_init", "vx_split_claim", "vx_split_done", "vx_split_boundary", "vx_verify_files_split",
    "vx_verify_files_split_multi",
    "vx_merkle_device_uniform", "vx_merkle_device_ragged", "vx_merkle_device_root", "vx_merkle_pad_hash",
    "vx_merkle_verify_batch",
    "vx_merkle_device_blocks", "vx_merkle_device_nodes", "vx_merkle_verify_files", "vx_merkle_verify_files_range",
    "vx_merkle_device_pieces", "vx_merkle_submit", "vx_merkle_poll",
    "vx_merkle_layers_plan", "vx_merkle_device_layers", "vx_merkle_device_proofs", "vx_merkle_verify_layers",
    "vx_merkle_verify_proofs",
    "vx_merkle_bitmap_words", "vx_merkle_device_block_check", "vx_merkle_check_blocks",
    "vx_hybrid_device_pieces", "vx_hybrid_verify_files", "vx_hybrid_verify_files_range",
    "vx_hybrid_submit", "vx_hybrid_set_piece_tables", "vx_hybrid_submit_piece", "vx_hybrid_poll",
    "vx_merkle_tree_rows", "vx_merkle_tree_plan", "vx_merkle_device_trees", "vx_merkle_build_trees",
    "vx_merkle_tree_proof", "vx_merkle_tree_layout",
    "vx_hash_files", "vx_hash_files_range", "vx_merkle_hash_files", "vx_merkle_hash_files_range",
    "vx_hybrid_hash_files", "vx_hybrid_hash_files_range",
    "vx_set_skip_holes", "vx_last_verify_holes", "vx_sha1_device_zeros", "vx_merkle_device_zero_leaves",
    "vx_merkle_leaf_rows", "vx_merkle_device_leaf_check", "vx_merkle_verify_files_blocks",
    "vx_merkle_verify_files_blocks_range", "vx_merkle_hash_files_leaves", "vx_merkle_hash_files_leaves_range",
    "vx_set_merkle_zero_copy", "vx_merkle_zero_copy_trace",
)
# ... plus include/vx_tuning.h and include/vx_synth.h: libvortex_amd_tuning.so only.
TUNING_EXPORTS = (
    "vx_synth_fill", "vx_sha1_device_uniform_variant", "vx_sha1_device_ragged_variant",
    "vx_tuning_zero_copy_plan", "vx_tuning_zero_copy_kernel", "vx_tuning_plan_ragged", "vx_tuning_chunk_schedule",
    "vx_tuning_fail_submit_after", "vx_tuning_fail_launch_after", "vx_tuning_verify_copy_stream", "vx_tuning_stage_huge",
    "vx_tuning_live_resources", "vx_tuning_fail_alloc_after",
    "vx_tuning_split_rules", "vx_tuning_clock_stamp",
    "vx_tuning_wall_clock_khz", "vx_tuning_device_identity", "vx_tuning_split_take_tail",
    "vx_tuning_last_split", "vx_tuning_zero_tail_kernel", "vx_tuning_chunk_kernel",
    "vx_tuning_hybrid_finish_kernel", "vx_tuning_zero_run_kernel", "vx_tuning_zero_leaf_kernel",
    "vx_tuning_gather_kernel", "vx_tuning_merkle_zc_kernel", "vx_tuning_merkle_zc_geometry",
)


class VxError(RuntimeError):
    def __init__(self, code: int, where: str, msg: str):
        super().__init__(f"{where} failed: {code} ({msg})")
        self.code = code
        # HashPool.spawn: (index, conn_id, buffer) of a piece the engine did not take
        self.refused = None


class vx_completion(ctypes.Structure):
    _fields_ = [("tag", ctypes.c_uint64), ("matched", ctypes.c_uint8), ("digest", ctypes.c_uint8 * 20),
                ("_pad", ctypes.c_uint8 * 3)]


class vx_merkle_completion(ctypes.Structure):
    """A v2 piece's completion (vx_merkle_poll): 48 bytes."""
    _fields_ = [("tag", ctypes.c_uint64), ("matched", ctypes.c_uint8), ("root", ctypes.c_uint8 * 32),
                ("_pad", ctypes.c_uint8 * 7)]


class vx_hybrid_completion(ctypes.Structure):
    """A hybrid piece's completion (vx_hybrid_poll): 64 bytes; matched bit 0 = SHA-1, bit 1 = root."""
    _fields_ = [("tag", ctypes.c_uint64), ("matched", ctypes.c_uint8), ("_pad", ctypes.c_uint8 * 3),
                ("sha1", ctypes.c_uint8 * 20), ("root", ctypes.c_uint8 * 32)]


VX_MERKLE_TILE_ROWS = 512


class vx_merkle_tile(ctypes.Structure):
    """One workgroup in one pass of vx_merkle_device_layers: 16 bytes."""
    _fields_ = [("in_row", ctypes.c_uint32), ("out", ctypes.c_uint32), ("rows", ctypes.c_uint16),
                ("levels", ctypes.c_uint8), ("last", ctypes.c_uint8), ("_pad", ctypes.c_uint32)]


class vx_merkle_layers_plan(ctypes.Structure):
    """What vx_merkle_layers_plan (the function) fills: 48 bytes.  In C the
    struct goes by its tag, `struct vx_merkle_layers_plan`."""
    _fields_ = [("n_layers", ctypes.c_uint32), ("passes", ctypes.c_uint32), ("rows", ctypes.c_uint64),
                ("work_rows", ctypes.c_uint64), ("n_tiles", ctypes.c_uint32), ("pass_tiles", ctypes.c_uint32 * 4),
                ("_pad", ctypes.c_uint32)]


class vx_merkle_tree_tile(ctypes.Structure):
    """One workgroup in one pass of vx_merkle_device_trees: 16 bytes."""
    _fields_ = [("src_row", ctypes.c_uint32), ("dst_row", ctypes.c_uint32), ("level_rows", ctypes.c_uint32),
                ("tile", ctypes.c_uint32)]


class vx_merkle_tree_plan(ctypes.Structure):
    """What vx_merkle_tree_plan (the function) fills: 48 bytes.  In C the
    struct goes by its tag, `struct vx_merkle_tree_plan`."""
    _fields_ = [("n_layers", ctypes.c_uint32), ("passes", ctypes.c_uint32), ("rows", ctypes.c_uint64),
                ("tree_rows", ctypes.c_uint64), ("n_tiles", ctypes.c_uint32), ("pass_tiles", ctypes.c_uint32 * 4),
                ("_pad", ctypes.c_uint32)]


class vx_merkle_proof(ctypes.Structure):
    """One hash proof (a BEP 52 `hashes` message): 24 bytes."""
    _fields_ = [("pos", ctypes.c_uint64), ("row", ctypes.c_uint32), ("expected", ctypes.c_uint32),
                ("span", ctypes.c_uint16), ("uncles", ctypes.c_uint8), ("_pad", ctypes.c_uint8 * 5)]


def proof_array(proofs):
    """A host sequence of proofs, each (pos, row, expected, span, uncles) or a
    vx_merkle_proof, as a ctypes array; ValueError when a number does not fit
    its field (ctypes would cut it silently)."""
    arr = (vx_merkle_proof * max(len(proofs), 1))()
    widths = (64, 32, 32, 16, 8)
    for i, p in enumerate(proofs):
        v = (p.pos, p.row, p.expected, p.span, p.uncles) if isinstance(p, vx_merkle_proof) else tuple(int(x) for x in p)
        if len(v) != 5 or any(not 0 <= x < 1 << w for x, w in zip(v, widths)):
            raise ValueError(f"proof {i}: (pos, row, expected, span, uncles) = {v} does not fit vx_merkle_proof")
        arr[i].pos, arr[i].row, arr[i].expected, arr[i].span, arr[i].uncles = v
    return arr


ABI_VERSION = 3

# vx_config fields a caller may set beyond the pool geometry (ABI 2; include/vx_hash.h)
CONFIG_OPTIONS = ("zero_copy", "direct_io", "batch_chunk", "verify_chunk", "verify_cold_chunk", "verify_ramp",
                  "refuse_when_full")


class vx_config(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("max_piece_len", ctypes.c_uint32), ("batch_pieces", ctypes.c_uint32),
                ("slots", ctypes.c_uint32), ("slot_bytes", ctypes.c_uint64)] + \
        [(name, ctypes.c_uint32) for name in CONFIG_OPTIONS]


class vx_plan(ctypes.Structure):
    _fields_ = [("gpu_s", ctypes.c_double), ("gpu_chain_s", ctypes.c_double), ("gpu_transfer_s", ctypes.c_double),
                ("cpu_s", ctypes.c_double), ("piece_latency_s", ctypes.c_double),
                ("cpu_piece_latency_s", ctypes.c_double), ("use_gpu", ctypes.c_int32), ("_pad", ctypes.c_uint32)]


VX_STATS_HIST = 24


class vx_stats(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in (
        "pieces_completed", "pieces_mismatched", "bytes_completed", "batches", "chunk_rounds", "gather_tiles",
        "staged_bytes", "io_errors", "submit_stall_ns", "batch_latency_count", "batch_latency_sum_us",
        "batch_latency_max_us")] + [("batch_latency_hist", ctypes.c_uint64 * VX_STATS_HIST)] + [
        (name, ctypes.c_uint64) for name in ("zero_copy_slots", "zero_copy_loader_slots", "submits_refused")]


class vx_verify_trace(ctypes.Structure):
    _fields_ = [(name, ctypes.c_double) for name in (
        "wall_ms", "read_busy_ms", "read_span_ms", "first_read_ms", "copy_busy_ms", "copy_span_ms", "tail_ms")] + [
        ("read_bytes", ctypes.c_uint64), ("copy_bytes", ctypes.c_uint64), ("readers", ctypes.c_uint32),
        ("rounds", ctypes.c_uint32), ("direct_bytes", ctypes.c_uint64),
        ("chunk_bytes", ctypes.c_uint64)]


class vx_hole_trace(ctypes.Structure):
    """What the last file re-verify skipped (vx_last_verify_holes): 48 bytes."""
    _fields_ = [(name, ctypes.c_uint64) for name in ("hole_pieces", "hole_blocks", "hole_bytes", "extents")] + [
        ("scan_ms", ctypes.c_double), ("zero_hash_ms", ctypes.c_double)]


MERKLE_ZC_TRACE_FIELDS = ("slots", "pieces", "bytes", "fallback_slots")
_made = {}


def merkle_zc_trace_type():
    """The ctypes form of vx_merkle_zc_trace (vx_merkle_zero_copy_trace): four
    uint64_t, 32 bytes.  In C the struct has no tag, only its typedef, so it is
    not one of the module's tagged structures; made on first use, and its
    layout is checked against the header by tests/test_merkle_zc_cpu.py."""
    if "vx_merkle_zc_trace" not in _made:
        _made["vx_merkle_zc_trace"] = type("vx_merkle_zc_trace", (ctypes.Structure,),
                                           {"_fields_": [(name, ctypes.c_uint64) for name in MERKLE_ZC_TRACE_FIELDS]})
    return _made["vx_merkle_zc_trace"]


VX_ROUND_NEW_WINDOW, VX_ROUND_HEAD_RAMP, VX_ROUND_TAIL_RAMP = 1, 2, 4


class vx_verify_round(ctypes.Structure):
    _fields_ = [(name, ctypes.c_double) for name in (
        "read_submit_ms", "read_done_ms", "enqueue_ms", "copy_start_ms", "copy_end_ms", "kernel_end_ms")] + [
        ("bytes", ctypes.c_uint64), ("offset", ctypes.c_uint64), ("lanes", ctypes.c_uint32),
        ("flags", ctypes.c_uint32)]


class vx_split(ctypes.Structure):
    """The split's claim word and the pool's progress (include/vx_hash.h)."""
    _fields_ = [("word", ctypes.c_uint64), ("pool_done", ctypes.c_uint64), ("start_ns", ctypes.c_uint64),
                ("first", ctypes.c_uint64), ("end", ctypes.c_uint64), ("cpu_threads", ctypes.c_uint32),
                ("engines", ctypes.c_uint32), ("cpu_thread_rate", ctypes.c_double),
                ("pool_last_ns", ctypes.c_uint64)]


_lib = None
_tuning = None
_lock = threading.Lock()


def _declare(L: ctypes.CDLL, tuning: bool = False) -> None:
    c = ctypes
    vp = c.c_void_p
    sig = {
        "vx_abi_version": ([], c.c_int),
        "vx_last_error": ([], c.c_char_p),
        "vx_strerror": ([c.c_int], c.c_char_p),
        "vx_device_count": ([], c.c_int),
        "vx_config_default": ([c.POINTER(vx_config), c.c_uint32], None),
        "vx_create": ([c.POINTER(vx_config), c.POINTER(vp)], c.c_int),
        "vx_destroy": ([vp], c.c_int),
        "vx_register_host_buffer": ([vp, vp, c.c_size_t], c.c_int),
        "vx_unregister_host_buffer": ([vp, vp], c.c_int),
        "vx_submit": ([vp, c.c_uint64, vp, c.c_uint32, vp], c.c_int),
        "vx_flush": ([vp], c.c_int),
        "vx_set_piece_table": ([vp, vp, c.c_uint32], c.c_int),
        "vx_submit_piece": ([vp, c.c_uint64, vp, c.c_uint32, c.c_uint32], c.c_int),
        "vx_poll": ([vp, c.POINTER(vx_completion), c.c_size_t], c.c_int64),
        "vx_drain": ([vp, c.c_uint32], c.c_int),
        "vx_pending": ([vp], c.c_uint64),
        "vx_get_stats": ([vp, c.POINTER(vx_stats)], c.c_int),
        "vx_reset_stats": ([vp], c.c_int),
        "vx_sha1_batch": ([vp, vp, vp, c.c_size_t, vp], c.c_int),
        "vx_verify_batch": ([vp, vp, vp, vp, c.c_size_t, vp, vp], c.c_int),
        "vx_verify_files": ([vp, vp, vp, c.c_size_t, c.c_uint32, vp, c.c_size_t, vp, c.c_uint32], c.c_int64),
        "vx_verify_files_range": ([vp, vp, vp, c.c_size_t, c.c_uint32, vp, c.c_size_t, c.c_size_t, c.c_size_t, vp,
                                   c.c_uint32], c.c_int64),
        "vx_verify_files_multi": ([vp, c.c_size_t, vp, vp, c.c_size_t, c.c_uint32, vp, c.c_size_t, vp, c.c_uint32],
                                  c.c_int64),
        "vx_sha1_device_uniform": ([vp, c.c_uint64, c.c_uint32, c.c_uint32, vp, vp, vp, vp], c.c_int),
        "vx_sha1_device_ragged": ([vp, vp, vp, vp, c.c_uint32, vp, vp, vp, vp], c.c_int),
        "vx_sha1_device_ragged_hint": ([vp, vp, vp, vp, c.c_uint32, c.c_uint32, c.c_uint64, vp, vp, vp, vp],
                                       c.c_int),
        "vx_sort_order": ([vp, c.c_uint32, vp], c.c_int),
        "vx_last_verify": ([vp, c.POINTER(vx_verify_trace)], c.c_int),
        "vx_last_verify_rounds": ([vp, c.POINTER(vx_verify_round), c.c_size_t], c.c_int64),
        "vx_set_skip_holes": ([vp, c.c_int], c.c_int),
        "vx_last_verify_holes": ([vp, c.POINTER(vx_hole_trace)], c.c_int),
        "vx_set_merkle_zero_copy": ([vp, c.c_int], c.c_int),
        "vx_merkle_zero_copy_trace": ([vp, c.POINTER(merkle_zc_trace_type())], c.c_int),
        "vx_sha1_device_zeros": ([vp, c.c_uint32, vp, vp], c.c_int),
        "vx_merkle_device_zero_leaves": ([vp, c.c_uint32, vp, vp], c.c_int),
        "vx_plan_verify": ([c.c_uint64, c.c_uint32, c.c_uint64, c.c_uint32, c.c_double, c.POINTER(vx_plan)], c.c_int),
        "vx_plan_verify_gpus": ([c.c_uint64, c.c_uint32, c.c_uint64, c.c_uint32, c.c_double, c.c_uint32,
                                 c.POINTER(vx_plan)], c.c_int),
        "vx_plan_verify_split": ([c.c_uint64, c.c_uint32, c.c_uint64, c.c_uint32, c.c_double, c.c_uint32,
                                  c.POINTER(c.c_uint64), c.POINTER(c.c_uint64), c.POINTER(vx_plan)], c.c_int),
        "vx_split_init": ([c.POINTER(vx_split), c.c_uint64, c.c_uint64, c.c_uint32, c.c_double], c.c_int),
        "vx_split_claim": ([c.POINTER(vx_split)], c.c_int64),
        "vx_split_done": ([c.POINTER(vx_split), c.c_uint64], None),
        "vx_split_boundary": ([c.POINTER(vx_split)], c.c_uint64),
        "vx_verify_files_split": ([vp, vp, vp, c.c_size_t, c.c_uint32, vp, c.c_size_t, c.POINTER(vx_split), vp,
                                   c.c_uint32], c.c_int64),
        "vx_verify_files_split_multi": ([vp, c.c_size_t, vp, vp, c.c_size_t, c.c_uint32, vp, c.c_size_t,
                                         c.POINTER(vx_split), vp, c.c_uint32], c.c_int64),
        "vx_merkle_device_uniform": ([vp, c.c_uint64, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp, vp, vp,
                                      vp], c.c_int),
        "vx_merkle_device_ragged": ([vp, vp, vp, vp, c.c_uint32, c.c_uint32, vp, vp, vp, vp, vp], c.c_int),
        "vx_merkle_device_root": ([vp, c.c_uint32, c.c_uint32, vp, vp, vp], c.c_int),
        "vx_merkle_pad_hash": ([c.c_uint32, vp], c.c_int),
        "vx_merkle_verify_batch": ([vp, vp, vp, vp, c.c_size_t, c.c_uint32, vp, vp, vp], c.c_int),
        "vx_merkle_device_blocks": ([vp, vp, vp, c.c_uint32, vp, vp], c.c_int),
        "vx_merkle_device_nodes": ([vp, vp, c.c_uint32, c.c_uint32, vp, vp, vp, vp], c.c_int),
        "vx_merkle_verify_files": ([vp, vp, vp, c.c_size_t, c.c_uint32, vp, c.c_size_t, vp, c.c_uint32], c.c_int64),
        "vx_merkle_verify_files_range": ([vp, vp, vp, c.c_size_t, c.c_uint32, vp, c.c_size_t, c.c_size_t,
                                          c.c_size_t, vp, c.c_uint32], c.c_int64),
        "vx_merkle_device_pieces": ([vp, vp, vp, vp, c.c_uint32, c.c_uint32, vp, vp, vp, vp, vp], c.c_int),
        "vx_merkle_submit": ([vp, c.c_uint64, vp, c.c_uint32, c.c_uint32, vp], c.c_int),
        "vx_merkle_poll": ([vp, c.POINTER(vx_merkle_completion), c.c_size_t], c.c_int64),
        "vx_merkle_layers_plan": ([vp, c.c_uint32, c.POINTER(vx_merkle_layers_plan), vp, c.c_size_t], c.c_int),
        "vx_merkle_device_layers": ([vp, c.POINTER(vx_merkle_layers_plan), vp, c.c_uint32, vp, vp, vp, vp, vp],
                                    c.c_int),
        "vx_merkle_device_proofs": ([vp, vp, c.c_uint32, vp, vp, vp, vp], c.c_int),
        "vx_merkle_verify_layers": ([vp, vp, vp, c.c_uint32, c.c_uint32, vp, vp, vp], c.c_int),
        "vx_merkle_verify_proofs": ([vp, vp, c.c_uint64, vp, c.c_uint32, vp, c.c_uint32, vp, vp], c.c_int),
        "vx_merkle_bitmap_words": ([c.c_uint32, c.c_uint32], c.c_uint64),
        "vx_merkle_device_block_check": ([vp, vp, vp, c.c_uint32, c.c_uint32, vp, vp, vp, vp], c.c_int),
        "vx_merkle_check_blocks": ([vp, vp, vp, c.c_size_t, c.c_uint32, vp, vp, vp, vp], c.c_int),
        "vx_hybrid_device_pieces": ([vp, vp, vp, vp, vp, c.c_uint32, c.c_uint32, vp, vp, vp, vp, vp, vp, vp], c.c_int),
        "vx_hybrid_verify_files": ([vp, vp, vp, c.c_size_t, c.c_uint32, vp, vp, c.c_size_t, vp, c.c_uint32],
                                   c.c_int64),
        "vx_hybrid_verify_files_range": ([vp, vp, vp, c.c_size_t, c.c_uint32, vp, vp, c.c_size_t, c.c_size_t,
                                          c.c_size_t, vp, c.c_uint32], c.c_int64),
        "vx_hybrid_submit": ([vp, c.c_uint64, vp, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp], c.c_int),
        "vx_hybrid_set_piece_tables": ([vp, vp, vp, c.c_uint32], c.c_int),
        "vx_hybrid_submit_piece": ([vp, c.c_uint64, vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32], c.c_int),
        "vx_hybrid_poll": ([vp, c.POINTER(vx_hybrid_completion), c.c_size_t], c.c_int64),
        "vx_merkle_tree_rows": ([c.c_uint64], c.c_uint64),
        "vx_merkle_tree_plan": ([vp, c.c_uint32, c.POINTER(vx_merkle_tree_plan), vp, c.c_size_t, vp], c.c_int),
        "vx_merkle_device_trees": ([vp, c.POINTER(vx_merkle_tree_plan), vp, c.c_uint32, vp, vp], c.c_int),
        "vx_merkle_build_trees": ([vp, vp, vp, c.c_uint32, c.c_uint32, vp, vp], c.c_int),
        "vx_merkle_tree_proof": ([vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint64, c.c_uint32, c.c_uint32, vp],
                                 c.c_int),
        "vx_merkle_tree_layout": ([vp, c.c_size_t, c.c_uint32, vp, vp], c.c_int64),
        "vx_hash_files": ([vp, vp, vp, c.c_size_t, c.c_uint32, c.c_size_t, vp, vp, c.c_uint32], c.c_int64),
        "vx_hash_files_range": ([vp, vp, vp, c.c_size_t, c.c_uint32, c.c_size_t, c.c_size_t, c.c_size_t, vp, vp,
                                 c.c_uint32], c.c_int64),
        "vx_merkle_hash_files": ([vp, vp, vp, c.c_size_t, c.c_uint32, c.c_size_t, vp, vp, vp, c.c_uint64,
                                  c.c_uint32], c.c_int64),
        "vx_merkle_hash_files_range": ([vp, vp, vp, c.c_size_t, c.c_uint32, c.c_size_t, c.c_size_t, c.c_size_t, vp,
                                        vp, c.c_uint32], c.c_int64),
        "vx_merkle_leaf_rows": ([vp, c.c_size_t, c.c_uint32], c.c_int64),
        "vx_merkle_device_leaf_check": ([vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp, vp, vp, vp, vp,
                                         vp], c.c_int),
        "vx_merkle_verify_files_blocks": ([vp, vp, vp, c.c_size_t, c.c_uint32, vp, c.c_size_t, vp, c.c_uint64, vp,
                                           vp, vp, vp, c.c_uint32], c.c_int64),
        "vx_merkle_verify_files_blocks_range": ([vp, vp, vp, c.c_size_t, c.c_uint32, vp, c.c_size_t, vp, c.c_uint64,
                                                 c.c_size_t, c.c_size_t, vp, vp, vp, vp, c.c_uint32], c.c_int64),
        "vx_merkle_hash_files_leaves": ([vp, vp, vp, c.c_size_t, c.c_uint32, c.c_size_t, vp, vp, vp, c.c_uint64, vp,
                                         c.c_uint64, c.c_uint32], c.c_int64),
        "vx_merkle_hash_files_leaves_range": ([vp, vp, vp, c.c_size_t, c.c_uint32, c.c_size_t, c.c_size_t,
                                               c.c_size_t, vp, vp, vp, c.c_uint64, c.c_uint32], c.c_int64),
        "vx_hybrid_hash_files": ([vp, vp, vp, c.c_size_t, c.c_uint32, c.c_size_t, vp, vp, vp, vp, c.c_uint64,
                                  c.c_uint32], c.c_int64),
        "vx_hybrid_hash_files_range": ([vp, vp, vp, c.c_size_t, c.c_uint32, c.c_size_t, c.c_size_t, c.c_size_t, vp,
                                        vp, vp, c.c_uint32], c.c_int64),
    }
    if tuning:
        sig.update({
            "vx_sha1_device_uniform_variant": ([vp, c.c_uint64, c.c_uint32, c.c_uint32, vp, vp, vp, vp, c.c_int],
                                               c.c_int),
            "vx_sha1_device_ragged_variant": ([vp, vp, vp, vp, c.c_uint32, vp, vp, vp, vp, c.c_int], c.c_int),
            "vx_tuning_zero_copy_plan": ([c.c_uint32, c.c_uint64], c.c_int),
            "vx_tuning_zero_copy_kernel": ([vp, vp, c.c_uint32, vp, vp, vp, c.c_int, vp], c.c_int),
            "vx_tuning_zero_tail_kernel": ([vp, vp, vp, vp, c.c_uint32, c.c_uint64, vp, vp, vp], c.c_int),
            "vx_tuning_chunk_kernel": ([vp, vp, vp, c.c_uint32, vp, vp, vp, vp, vp, vp], c.c_int),
            "vx_tuning_hybrid_finish_kernel": ([vp, vp, vp, vp, c.c_uint32, c.c_uint64, vp, vp, vp, vp, vp, vp, vp,
                                                vp, vp], c.c_int),
            "vx_tuning_zero_run_kernel": ([vp, vp, vp, c.c_uint32, vp, vp], c.c_int),
            "vx_tuning_zero_leaf_kernel": ([vp, vp, c.c_uint32, vp, vp, vp], c.c_int),
            "vx_tuning_gather_kernel": ([vp, vp, vp, vp, c.c_uint32, c.c_uint32, vp, c.c_uint32, vp], c.c_int),
            "vx_tuning_merkle_zc_kernel": ([vp, vp, vp, c.c_uint32, c.c_uint32, vp, vp, vp, vp], c.c_int),
            "vx_tuning_merkle_zc_geometry": ([c.POINTER(c.c_uint32)], None),
            "vx_tuning_fail_submit_after": ([vp, c.c_int64], None),
            "vx_tuning_fail_launch_after": ([vp, c.c_int64], None),
            "vx_tuning_verify_copy_stream": ([vp, c.c_int], None),
            "vx_tuning_stage_huge": ([vp, c.c_int], None),
            "vx_tuning_live_resources": ([vp], None),
            "vx_tuning_fail_alloc_after": ([c.c_int64], None),
            "vx_tuning_split_rules": ([vp, c.c_int, c.c_uint64, c.c_int, c.c_int], None),
            "vx_tuning_clock_stamp": ([vp, c.c_uint32, vp], c.c_int),
            "vx_tuning_wall_clock_khz": ([c.c_int], c.c_int),
            "vx_tuning_device_identity": ([c.c_int, c.c_char_p, c.c_size_t, c.c_char_p], c.c_int),
            "vx_tuning_plan_ragged": ([c.c_uint32, c.c_uint32, c.c_uint64], c.c_int),
            "vx_tuning_split_take_tail": ([c.POINTER(vx_split), c.c_uint64, c.POINTER(c.c_uint64)], c.c_uint64),
            "vx_tuning_last_split": ([vp, c.POINTER(c.c_double), c.c_size_t], c.c_size_t),
            "vx_tuning_chunk_schedule": ([c.c_uint64, c.c_uint64, c.c_int, c.c_int, c.POINTER(c.c_uint64),
                                          c.c_size_t], c.c_size_t),
            "vx_synth_fill": ([vp, c.c_uint64, c.c_uint32, c.c_uint32, c.c_uint64, c.c_uint64, c.c_uint32, vp],
                              c.c_int),
        })
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res


def _load(path: str, tuning: bool) -> ctypes.CDLL:
    import torch  # noqa: F401  (single HIP runtime, see module doc)

    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the HIP engine is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C vortex_amd/csrc`).")
    L = ctypes.CDLL(path)
    _declare(L, tuning)
    if L.vx_abi_version() != ABI_VERSION:
        raise ImportError(f"{os.path.basename(path)} ABI version mismatch")
    return L


def lib() -> ctypes.CDLL:
    """Load libvortex_amd.so once; raise ImportError if it was never built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            _lib = _load(LIB_PATH, False)
    return _lib


def tuning() -> ctypes.CDLL:
    """Load libvortex_amd_tuning.so once (tests, bench.py; vx_tuning.h)."""
    global _tuning
    if _tuning is not None:
        return _tuning
    with _lock:
        if _tuning is None:
            _tuning = _load(TUNING_PATH, True)
    return _tuning


def check(rc: int, where: str, L: ctypes.CDLL | None = None) -> int:
    """Raise VxError for a negative code; the message is the thread-local
    vx_last_error of the library that failed (L, default lib())."""
    if rc < 0:
        msg = (L or lib()).vx_last_error().decode(errors="replace")
        raise VxError(rc, where, msg)
    return rc
