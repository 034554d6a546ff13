"""GPU: the hybrid re-verify over file holes (HashPool.skip_holes with
verify_hybrid_files), over the sparse torrents of
tests/_hybrid_sparse.py.

Chunks the file system never wrote are judged without a read: the verdict
bytes, the I/O errors and the stats must be those of the setting off and of
hashlib over what the files hold, and the hole counts and read_bytes those of
the os.lseek model (vortex_amd/sparse.py).  The setting is on for the first
call over a torrent's files: a fallocated range that has been read through the
page cache can report as data afterwards.

Every test makes its verdict assertions first; where the file system reports
no holes the count assertions do not apply."""
import pytest

import _hybrid_sparse as hs
from _sparse import NO_HOLES, holes_reported

pytestmark = pytest.mark.gpu

KEYS = ("pieces_completed", "pieces_mismatched", "bytes_completed", "io_errors")


def _verdicts(res):
    return [int(a) | int(b) << 1 for a, b in res]


def _call(pool, t, skip, **kw):
    """One verify_hybrid_files call: (verdict bytes, stats delta, hole trace, read_bytes)."""
    pool.skip_holes = skip
    pool.reset_stats()
    res = pool.verify_hybrid_files(t["paths"], t["flens"], t["pl"], t["exp1"], t["exp2"], **kw)
    st = pool.stats()
    return _verdicts(res), {k: st[k] for k in KEYS}, pool.last_verify_holes(), pool.last_verify()["read_bytes"]


@pytest.fixture(scope="module")
def runs(built, gpu, tmp_path_factory):
    """Every torrent verified with the setting on (first: the files are fresh),
    on again, and off, on one context; and the model's figures, scanned first."""
    from vortex_amd import sparse
    from vortex_amd.hash_pool import HashPool

    d = tmp_path_factory.mktemp("hsparse_gpu")
    ts = hs.all_torrents(d)
    out = {}
    with HashPool(hs.PL) as pool:
        for t in ts:
            model = sparse.hybrid_read_bytes(t["paths"], t["flens"], t["pl"])
            on = _call(pool, t, True)
            again = _call(pool, t, True)
            off = _call(pool, t, False)
            out[t["name"]] = dict(t=t, model=model, on=on, again=again, off=off)
    return out, holes_reported(d)


@pytest.mark.parametrize("name", ["main", "last-trailing", "last-whole", "last-leading", "short-on-disk", "256KiB"])
def test_verdicts_and_stats_equal_off_on_and_hashlib(runs, name):
    r = runs[0][name]
    t, on, off = r["t"], r["on"], r["off"]
    assert off[0] == t["want"], "setting off"
    assert on[0] == t["want"], "setting on"
    assert r["again"][0] == t["want"]
    n = len(t["want"])
    want_stats = dict(pieces_completed=n, pieces_mismatched=sum(v != 3 for v in t["want"]) - t["io_errors"],
                      bytes_completed=sum(t["flens"]), io_errors=t["io_errors"])
    assert off[1] == want_stats and on[1] == want_stats
    assert off[2] == dict.fromkeys(off[2], 0), "nothing is scanned or skipped with the setting off"
    if not t["io_errors"]:
        assert off[3] == sum(t["flens"])


def test_hole_pieces_get_every_verdict(runs):
    """Pieces of zeros (unwritten, whole): right rows give 3, a wrong SHA-1 row
    with the right root 2, the reverse 1."""
    got = {}
    for r in runs[0].values():
        for i, v in hs.zero_verdicts(r["t"]):
            assert r["on"][0][i] == v
            got.setdefault(v, []).append((r["t"]["name"], i))
    assert {1, 2, 3} <= set(got)


@pytest.mark.parametrize("name", ["main", "last-trailing", "last-whole", "last-leading", "short-on-disk", "256KiB"])
def test_hole_counters_and_read_bytes_equal_the_model(runs, name):
    if not runs[1]:
        pytest.skip(NO_HOLES)
    r = runs[0][name]
    t, m, (_, _, trace, read_bytes) = r["t"], r["model"], r["on"]
    for key in ("hole_pieces", "hole_blocks", "hole_bytes", "extents"):
        assert trace[key] == m[key], key
    if not t["io_errors"]:
        assert read_bytes == m["read_bytes"] and read_bytes + trace["hole_bytes"] == sum(t["flens"])
    assert trace["scan_ms"] > 0
    assert r["off"][3] - read_bytes == trace["hole_bytes"], "the setting saves the hole chunks' reads, nothing else"
    # a second call on the context finds the zero hashes it needs in the context
    assert r["again"][2]["zero_hash_ms"] == 0
    if name == "main":
        assert trace["hole_pieces"] == 5 and trace["zero_hash_ms"] > 0
        assert trace["hole_bytes"] == 32 * hs.C + sum(
            min(hs.C, k * hs.C + hs.TAIL - j * hs.C) for k in range(4) for msk in range(1 << (k + 1))
            for j in range(k + 1) if msk >> j & 1)
    if name == "last-trailing":
        assert trace["hole_bytes"] == 0 and read_bytes == sum(t["flens"]), "the last piece's trailing run is read"


def test_range_calls(built, gpu, tmp_path):
    """Ranges that start inside file 0, inside a run of hole chunks and at a
    whole-hole piece: the full call's verdicts, the model's counts."""
    from vortex_amd import sparse
    from vortex_amd.hash_pool import HashPool

    t = hs.main_torrent(tmp_path)
    ranges = [(5, 20), (15, 3), (44, 3)]
    models = [sparse.hybrid_read_bytes(t["paths"], t["flens"], t["pl"], first=f, count=c) for f, c in ranges]
    with HashPool(hs.PL, slots=3) as pool:
        got = [_call(pool, t, True, first=f, count=c) for f, c in ranges]
    for (f, c), g in zip(ranges, got):
        assert g[0] == t["want"][f:f + c], (f, c)
    if not holes_reported(tmp_path):
        pytest.skip(NO_HOLES)
    for (f, c), g, m in zip(ranges, got, models):
        assert g[3] == m["read_bytes"] and g[2]["hole_bytes"] == m["hole_bytes"], (f, c)
        assert g[2]["hole_pieces"] == m["hole_pieces"] and g[2]["hole_blocks"] == m["hole_blocks"], (f, c)


def test_hash_call_ignores_the_setting(built, gpu, tmp_path):
    """hash_hybrid_files with the setting on returns the tables it returns with
    it off, those of hashlib, and reports no holes."""
    from vortex_amd import hybrid
    from vortex_amd.hash_pool import HashPool

    t = hs.last_piece_torrents(tmp_path)[2]
    with HashPool(hs.PL) as pool:
        pool.skip_holes = True
        on = pool.hash_hybrid_files(t["paths"], t["flens"], t["pl"])
        trace, read_on = pool.last_verify_holes(), pool.last_verify()["read_bytes"]
        pool.skip_holes = False
        off = pool.hash_hybrid_files(t["paths"], t["flens"], t["pl"])
    assert on == off and trace == dict.fromkeys(trace, 0) and read_on == sum(t["flens"])
    findex, foff, dlen, pads, log2w = hybrid.hybrid_pieces(t["flens"], t["pl"])
    for i, (f, o, n, pad, lw) in enumerate(zip(findex, foff, dlen, pads, log2w)):
        data = t["content"][f][o:o + n]
        assert on[0][20 * i:20 * i + 20] == hybrid.v1_digest(data, pad), i
        assert on[1][32 * i:32 * i + 32] == hybrid.v2_root(data, lw), i
