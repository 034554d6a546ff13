"""GPU: a context gives back everything it took (vortex_amd/csrc/vx_resources.hpp,
DESIGN.md §6 "Ownership").

The test build counts the device blocks, pinned blocks (stages included),
streams and events the engine holds (vx_tuning_live_resources) and can fail
one creation on the host, before the runtime is asked
(vx_tuning_fail_alloc_after).  Per call family: the counts after the pool is
closed equal those before it was created
  B1  after one good run, its results checked against hashlib,
  B2  after an injected launch or submit failure,
  B3  after an allocation failure at every creation from the first of
      vx_create on, one per run.
Every failure is an error return made on the host: nothing is launched with a
missing buffer and nothing provokes a device fault.

The smallest shapes that reach every owner: contexts of 2 slots of 1 MiB, a
torrent of three files (394,216 + 70,000 + 5,000 bytes, the first with a 256
KiB hole) at 16 KiB and 64 KiB pieces.  In B3 the stages are not huge-page
mappings (vx_tuning_stage_huge 0): a refused registration falls back to pinned
memory without an error, which would end a sweep before the owners behind it
are reached."""
import ctypes
import hashlib
import mmap

import numpy as np
import pytest

from _sparse import NO_HOLES, holes_reported, make_file

pytestmark = pytest.mark.gpu

KiB = 1024
BLOCK = 16 * KiB
FLENS = (6 * 64 * KiB + 1000, 70000, 5000)
HOLE = (64 * KiB, 5 * 64 * KiB)  # of file 0, never written


def sha1(b):
    return hashlib.sha1(b).digest()


def live(L):
    out = (ctypes.c_uint64 * 4)()
    L.vx_tuning_live_resources(out)
    return list(out)


@pytest.fixture(scope="module")
def lib(built, gpu):
    from vortex_amd import _lib

    return _lib.tuning()


@pytest.fixture(scope="module")
def files(built, gpu, tmp_path_factory):
    """The three files on disk and what they hold."""
    root = tmp_path_factory.mktemp("resources")
    rng = np.random.default_rng(2024)
    content = [bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for n in FLENS]
    content[0][HOLE[0]:HOLE[1]] = bytes(HOLE[1] - HOLE[0])
    content = [bytes(c) for c in content]
    paths = [make_file(root / "f0", FLENS[0], [(0, content[0][:HOLE[0]]), (HOLE[1], content[0][HOLE[1]:])])]
    paths += [make_file(root / f"f{k}", FLENS[k], [(0, content[k])]) for k in (1, 2)]
    return {"paths": paths, "content": content, "holes": holes_reported(root)}


_TABLES = {}


def torrent(files, pl):
    """The torrent's tables at piece length pl, computed once with hashlib: v1
    (the files end to end), v2 and hybrid (file by file, vortex_amd.merkle and
    .hybrid), and per file its v2 layer and tree."""
    from vortex_amd import hybrid, merkle

    if pl in _TABLES:
        return _TABLES[pl]
    whole = b"".join(files["content"])
    v1 = [whole[o:o + pl] for o in range(0, len(whole), pl)]
    findex, foff, dlen, pads, log2w = hybrid.hybrid_pieces(FLENS, pl)
    v2 = [files["content"][f][o:o + n] for f, o, n in zip(findex, foff, dlen)]
    roots = [hybrid.v2_root(b, lw) for b, lw in zip(v2, log2w)]
    height = merkle.log2_width(pl)
    layers = [b"".join(r for r, f in zip(roots, findex) if f == k) for k in range(len(FLENS))]
    t = {"pl": pl, "paths": files["paths"], "flens": list(FLENS), "v1": v1, "sha1": [sha1(b) for b in v1],
         "v2": v2, "log2w": log2w, "pads": pads, "roots": roots, "height": height, "layers": layers,
         "hy_sha1": [hybrid.v1_digest(b, p) for b, p in zip(v2, pads)],
         "tree": b"".join(merkle.build_tree(layer, height) for layer in layers),
         "leaves": merkle.file_leaf_table(files["paths"], FLENS, pl)}
    _TABLES[pl] = t
    return t


class Pools:
    """The pools a family makes (2 slots of 1 MiB, the test build), closed by the test."""

    def __init__(self, after_create=None):
        self.made = []
        self.after_create = after_create  # (pool) -> None, right after vx_create

    def __call__(self, pl, **options):
        from vortex_amd.hash_pool import HashPool

        pool = HashPool(pl, slots=2, slot_bytes=1 << 20, batch_pieces=16, hooks=True, **options)
        self.made.append(pool)
        if self.after_create:
            self.after_create(pool)
        return pool

    def close(self):
        for pool in self.made:
            pool.close()


def wrong(rows, i):
    """rows with row i's first bit flipped: the one planted mismatch."""
    rows = list(rows)
    rows[i] = bytes([rows[i][0] ^ 1]) + rows[i][1:]
    return rows


# ---- the call families: each makes its pool(s), runs once and checks the results ----

def async_v1(t, pools):
    pool = pools(t["pl"])
    exp = wrong(t["sha1"], 2)
    for i, b in enumerate(t["v1"]):
        pool.spawn(i, 0, b, len(b), exp[i])
    pool.flush()
    pool.drain()
    got = {r.index: r for r in pool.try_iter()}
    assert sorted(got) == list(range(len(exp)))
    assert all(got[i].digest == t["sha1"][i] and got[i].hash_matched == (i != 2) for i in got)


def async_v2(t, pools):
    pool = pools(t["pl"])
    exp = wrong(t["roots"], 1)
    for i, b in enumerate(t["v2"]):
        pool.spawn_merkle(i, 0, b, len(b), exp[i], t["log2w"][i])
    pool.flush()
    pool.drain()
    got = {r.index: r for r in pool.try_iter_merkle()}
    assert sorted(got) == list(range(len(exp)))
    assert all(got[i].digest == t["roots"][i] and got[i].hash_matched == (i != 1) for i in got)


def async_hybrid(t, pools):
    pool = pools(t["pl"])
    n = len(t["v2"])
    pool.set_hybrid_tables(bytes(20 * n), bytes(32 * n))
    pool.set_hybrid_tables(b"".join(wrong(t["hy_sha1"], 0)), b"".join(wrong(t["roots"], 3)))  # replaces the first pair
    for i, b in enumerate(t["v2"]):
        pool.spawn_hybrid(i, 0, b, len(b), t["pads"][i], log2w=t["log2w"][i])
    pool.flush()
    pool.drain()
    got = {r.index: r for r in pool.try_iter_hybrid()}
    assert sorted(got) == list(range(n))
    for i in range(n):
        assert got[i].sha1 == t["hy_sha1"][i] and got[i].root == t["roots"][i], i
        assert got[i].matched == (2 if i == 0 else 1 if i == 3 else 3), i


def piece_table(t, pools):
    pool = pools(t["pl"])
    pool.set_piece_table(bytes(20 * len(t["sha1"])))
    pool.set_piece_table(b"".join(wrong(t["sha1"], 1)))  # replaces the first
    for i, b in enumerate(t["v1"]):
        pool.spawn(i, 0, b, len(b))
    pool.drain()
    got = {r.index: r for r in pool.try_iter()}
    assert all(got[i].digest == t["sha1"][i] and got[i].hash_matched == (i != 1) for i in range(len(t["sha1"])))


def registered(t, pools):
    pool = pools(t["pl"])
    pl, n = t["pl"], len(t["v1"])
    kept, reg = mmap.mmap(-1, 4096), mmap.mmap(-1, n * pl)
    pool.register_buffer(kept)  # still registered at close: vx_destroy's part
    pool.register_buffer(reg)
    for i, b in enumerate(t["v1"]):
        reg[i * pl:i * pl + len(b)] = b
        pool.spawn(i, 0, memoryview(reg)[i * pl:(i + 1) * pl], len(b), t["sha1"][i])
    pool.drain()
    got = {r.index: r for r in pool.try_iter()}
    pool.unregister_buffer(reg)
    assert all(got[i].digest == t["sha1"][i] and got[i].hash_matched for i in range(n))


def verify_batch(t, pools):
    verdicts, digests = pools(t["pl"]).verify_batch(t["v1"], wrong(t["sha1"], 0))
    assert digests == t["sha1"] and verdicts == [i != 0 for i in range(len(digests))]


def verify_merkle(t, pools):
    verdicts, roots = pools(t["pl"]).verify_merkle(t["v2"], wrong(t["roots"], 2), t["pl"], t["log2w"])
    assert roots == t["roots"] and verdicts == [i != 2 for i in range(len(roots))]


def verify_piece_layers(t, pools):
    from vortex_amd import merkle

    want = [merkle.layer_root(layer, t["height"]) for layer in t["layers"]]
    assert pools(t["pl"]).verify_piece_layers(t["layers"], wrong(want, 1), t["pl"]) == [True, False, True]


def verify_hash_proofs(t, pools):
    from vortex_amd import merkle

    layer, h = t["layers"][0], t["height"]
    n = len(layer) // 32
    uncles = (n - 1).bit_length() - 1
    rows = merkle.make_proof(layer, h, 1, 2, uncles) + merkle.make_proof(layer, h, 0, 2, uncles)
    proofs = [(1, 0, 0, 2, uncles), (0, 2 + uncles, 1, 2, uncles)]
    expected = [merkle.layer_root(layer, h), bytes(32)]
    assert pools(t["pl"]).verify_hash_proofs(rows, proofs, expected) == [True, False]


def check_blocks(t, pools):
    from vortex_amd import merkle

    pieces = t["v2"][:3]
    lw = t["height"]
    leaves = [merkle.leaf_rows(b, lw) for b in pieces]
    stale = [leaves[0], wrong([leaves[1]], 0)[0], leaves[2]]
    bad, got = pools(t["pl"]).check_blocks(pieces, t["pl"], stale, want_leaves=True)
    assert got == leaves and bad == [[], [0], []]


def build_piece_trees(t, pools):
    from vortex_amd import merkle

    trees, roots = pools(t["pl"]).build_piece_trees(t["layers"], t["pl"])
    want = [merkle.build_tree(layer, t["height"]) for layer in t["layers"]]
    assert trees == want and roots == [w[-32:] for w in want]


def verify_files(chunked, skip_holes):
    def run(t, pools):
        pool = pools(t["pl"], **({"verify_chunk": 16384} if chunked else {}))
        pool.skip_holes = skip_holes
        verdicts, io_errors = pool.verify_files(t["paths"], t["flens"], t["pl"], b"".join(wrong(t["sha1"], 0)))
        assert verdicts == [i != 0 for i in range(len(t["sha1"]))] and io_errors == 0
        assert (pool.stats()["chunk_rounds"] > 0) == chunked
    return run


def verify_merkle_files(t, pools):
    pool = pools(t["pl"])
    verdicts, io_errors = pool.verify_merkle_files(t["paths"], t["flens"], t["pl"], b"".join(wrong(t["roots"], 1)))
    assert verdicts == [i != 1 for i in range(len(t["roots"]))] and io_errors == 0


def verify_merkle_files_blocks(t, pools):
    pool = pools(t["pl"])
    stale = t["leaves"][:32] + bytes(32) + t["leaves"][64:]  # the stored row of block 1 of piece 0
    got = pool.verify_merkle_files_blocks(t["paths"], t["flens"], t["pl"], b"".join(t["roots"]), stale)
    n = len(t["roots"])
    assert got.matched == [True] * n and got.io_errors == 0
    assert got.layer_ok == [i != 0 for i in range(n)] and [got.blocks(i) for i in range(n)] == [[1]] + [[]] * (n - 1)


def hash_merkle_files_leaves(t, pools):
    rows, ok, tree, io_errors, leaves = pools(t["pl"]).hash_merkle_files_leaves(t["paths"], t["flens"], t["pl"])
    assert rows == b"".join(t["roots"]) and all(ok) and io_errors == 0
    assert tree == t["tree"] and leaves == t["leaves"]


def verify_hybrid_files(t, pools):
    pool = pools(t["pl"])
    pool.skip_holes = True
    got = pool.verify_hybrid_files(t["paths"], t["flens"], t["pl"], b"".join(wrong(t["hy_sha1"], 1)),
                                   b"".join(wrong(t["roots"], 2)))
    assert got == [(i != 1, i != 2) for i in range(len(t["roots"]))]


def hash_hybrid_files(t, pools):
    pieces, rows, ok, tree, io_errors = pools(t["pl"]).hash_hybrid_files(t["paths"], t["flens"], t["pl"])
    assert pieces == b"".join(t["hy_sha1"]) and rows == b"".join(t["roots"]) and all(ok) and io_errors == 0
    assert tree == t["tree"]


def verify_files_multi(t, pools):
    from vortex_amd.hash_pool import verify_files_multi as multi

    two = [pools(t["pl"], verify_chunk=16384), pools(t["pl"], verify_chunk=16384)]
    verdicts, io_errors = multi(two, t["paths"], t["flens"], t["pl"], b"".join(wrong(t["sha1"], 4)))
    assert verdicts == [i != 4 for i in range(len(t["sha1"]))] and io_errors == 0


# name: (piece length, the family, it reads file holes)
FAMILIES = {
    "async_v1": (16 * KiB, async_v1, False),
    "async_v2": (64 * KiB, async_v2, False),
    "async_hybrid": (64 * KiB, async_hybrid, False),
    "piece_table": (64 * KiB, piece_table, False),
    "registered": (16 * KiB, registered, False),
    "verify_batch": (64 * KiB, verify_batch, False),
    "verify_merkle": (64 * KiB, verify_merkle, False),
    "verify_piece_layers": (16 * KiB, verify_piece_layers, False),
    "verify_hash_proofs": (16 * KiB, verify_hash_proofs, False),
    "check_blocks": (64 * KiB, check_blocks, False),
    "build_piece_trees": (16 * KiB, build_piece_trees, False),
    "verify_files_whole": (16 * KiB, verify_files(False, False), False),
    "verify_files_whole_holes": (16 * KiB, verify_files(False, True), True),
    "verify_files_chunked": (64 * KiB, verify_files(True, False), False),
    "verify_files_chunked_holes": (64 * KiB, verify_files(True, True), True),
    "verify_merkle_files": (16 * KiB, verify_merkle_files, False),
    "verify_merkle_files_blocks": (64 * KiB, verify_merkle_files_blocks, False),
    "hash_merkle_files_leaves": (64 * KiB, hash_merkle_files_leaves, False),
    "verify_hybrid_files": (64 * KiB, verify_hybrid_files, True),
    "hash_hybrid_files": (16 * KiB, hash_hybrid_files, False),
    "verify_files_multi": (64 * KiB, verify_files_multi, False),
}


def family(files, name):
    pl, run, reads_holes = FAMILIES[name]
    if reads_holes and not files["holes"]:
        pytest.skip(NO_HOLES)
    return torrent(files, pl), run


@pytest.mark.parametrize("name", list(FAMILIES))
def test_a_context_returns_everything(lib, files, name):
    """B1: the counts before the pool is created, one good run of the family
    checked against hashlib, the pool closed, the same counts."""
    t, run = family(files, name)
    start = live(lib)
    pools = Pools()
    try:
        run(t, pools)
        held = live(lib)
    finally:
        pools.close()
    assert all(h > s for h, s in zip(held, start)), (start, held)  # the counters see the context
    assert live(lib) == start


@pytest.mark.parametrize("name", ["async_v1", "verify_files_chunked", "verify_merkle_files"])
def test_the_same_after_a_launch_failure(lib, files, name):
    """B2: the first launch (async), the first chunk round, the first block round
    fails as a device error does (vx_tuning_fail_launch_after 0): the call
    raises VX_EDEVICE as it did before, the pool is closed, the counts are back."""
    from vortex_amd._lib import VX_EDEVICE, VxError

    t, run = family(files, name)
    start = live(lib)
    pools = Pools(after_create=lambda pool: pool.lib.vx_tuning_fail_launch_after(pool._h, 0))
    try:
        with pytest.raises(VxError) as err:
            run(t, pools)
    finally:
        pools.close()
    assert err.value.code == VX_EDEVICE and "injected" in str(err.value) and "fail_launch_after" in str(err.value)
    assert live(lib) == start


# The creations on the longest path, vx_hybrid_verify_files over a hole: vx_create
# 12 (per slot a stream, 2 events, the arena and 2 metadata blocks), the holes' 5,
# HybridBufs 1 + 4 tables + 1 + the tail stream + 4 events, the run stream + 4
# events, the copy stream and 2 stages: 36.
CAP = 96


@pytest.mark.parametrize("name", ["create", "async_hybrid", "verify_merkle", "verify_files_chunked_holes",
                                  "verify_merkle_files_blocks", "verify_hybrid_files", "hash_merkle_files_leaves"])
def test_the_same_after_any_allocation_failure(lib, files, name):
    """B3: for k = 0, 1, ... the creation after k successful ones fails; the run
    ends well or with VX_ENOMEM / VX_EDEVICE, the pool (if there is one) is
    closed, the counts are back.  The sweep ends at the first k at which
    nothing failed, below CAP, having seen a failure inside vx_create and
    (but for "create", which only creates) one inside the call, above the last
    k that failed vx_create.  Then a fresh pool runs the family with correct
    results."""
    from vortex_amd._lib import VX_EDEVICE, VX_ENOMEM, VxError

    if name == "create":
        t, run = None, lambda t, pools: pools(64 * KiB)
    else:
        t, run = family(files, name)
    start = live(lib)
    in_create, in_call = [], []
    for k in range(CAP):
        pools = Pools(after_create=lambda pool: pool.lib.vx_tuning_stage_huge(pool._h, 0))
        failed = None
        lib.vx_tuning_fail_alloc_after(k)
        try:
            run(t, pools)
        except VxError as e:
            failed = e
        finally:
            lib.vx_tuning_fail_alloc_after(-1)
            pools.close()
        assert live(lib) == start, (k, str(failed))
        if failed is None:
            break
        assert failed.code in (VX_ENOMEM, VX_EDEVICE), (k, str(failed))
        (in_call if pools.made else in_create).append(k)
    else:
        pytest.fail(f"a creation still failed at k = {CAP - 1}")
    print(f"{name}: failed inside vx_create at k = {in_create}, inside the call at k = {in_call}")
    assert in_create, "no failure inside vx_create"
    if name != "create":
        assert in_call and min(in_call) > max(in_create), (in_create, in_call)
    pools = Pools()
    try:
        run(t, pools)
    finally:
        pools.close()
    assert live(lib) == start
