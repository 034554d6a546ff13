"""The proof sweep's batches (tests/_proof_sweep.py) are what
tests/test_gpu_proof_sweep.py says they are.  Host only: the tops are `walk`'s
(tests/test_merkle_layers_cpu.py), so what is checked here is which lanes hold
which descriptors, that every row a descriptor names is in bounds, and that
the wrong expected rows are wrong by exactly one bit each.
"""
import pytest

import _proof_sweep as ps


def _in_bounds(b):
    return all(row + span + uncles <= len(b.rows) and e < len(b.expected)
               for _, row, e, span, uncles in b.proofs)


@pytest.mark.parametrize("n", ps.SIZES)
def test_size_batches(n):
    b = ps.size_batch(n)
    assert b.n == n == len(b.tops) == len(b.expected) and _in_bounds(b)
    assert [p[3] for p in b.proofs] == [1 << (i % 10) for i in range(n)]
    assert any(p[4] == 64 and p[0] >> 63 for p in b.proofs)
    if n >= 63:
        assert {p[3] for p in b.proofs} == set(ps.SPANS) and {0, 1, 63, 64} <= {p[4] for p in b.proofs}
        assert any(p[0] >> 32 for p in b.proofs) and len({p[0] for p in b.proofs}) == n
    assert b.verdicts() == [1] * n
    # a span's root is the layer model's, and a proof of no uncles stops there
    i = next((i for i, p in enumerate(b.proofs) if p[4] == 0 and p[3] > 1), None)
    if i is not None:
        _, row, _, span, _ = b.proofs[i]
        assert b.tops[i] == ps.span_root(b.rows[row:row + span])


def test_sizes_sit_either_side_of_a_wave_and_of_a_workgroup():
    from _zero_sweep import LEAF_GROUP  # kBlock of vx_kernels.h: the walk kernel's workgroup

    assert LEAF_GROUP == 256 and ps.WAVE == 64
    assert set(ps.SIZES) >= {ps.WAVE - 1, ps.WAVE, ps.WAVE + 1, LEAF_GROUP - 1, LEAF_GROUP, LEAF_GROUP + 1, 1}
    assert max(ps.SIZES) > 2 * LEAF_GROUP and max(ps.SIZES) % ps.WAVE and sum(ps.SIZES) == 1561


def test_wave_shapes():
    counts = {k: [p[4] for p in ps.wave_batch(k).proofs] for k in ps.WAVE_SHAPES}
    assert all(len(c) == ps.WAVE_N == 130 for c in counts.values()) and ps.WAVE_N % ps.WAVE == 2
    assert set(counts["no uncles"]) == {0} and set(counts["all 64"]) == {64}
    assert [i for i, c in enumerate(counts["64 at lane 0"]) if c] == [0, 64, 128]
    assert [i for i, c in enumerate(counts["64 at lane 63"]) if c] == [63, 127]
    assert [i for i, c in enumerate(counts["64 at the last live lane"]) if c] == [129]
    assert counts["descending"][:64] == list(range(64, 0, -1)) and counts["descending"][128:] == [64, 63]
    assert counts["ascending"][:64] == list(range(1, 65)) and counts["ascending"][128:] == [1, 2]
    for k in ps.WAVE_SHAPES:
        b = ps.wave_batch(k)
        assert _in_bounds(b) and b.verdicts() == [1] * 130
        assert all(p[0] >> 63 for p in b.proofs if p[4] == 64)


def test_shared_rows():
    b = ps.shared_batch()
    assert _in_bounds(b) and len(b.rows) == 700
    assert sum(1 for p in b.proofs if p[1] == 0) >= 45 and sum(1 for p in b.proofs if p[2] == 0) == 40
    assert b.verdicts()[:25] == [1] * 25 and b.verdicts()[25:40] == [0] * 15 and b.verdicts()[40:] == [1] * 65
    spans = sorted((p[1], p[1] + p[3] + p[4]) for p in b.proofs[45:])
    assert sum(1 for (a0, a1), (b0, b1) in zip(spans, spans[1:]) if b0 < a1) >= 40, "ranges overlap"


def test_one_bit_rows():
    b = ps.one_bit_batch()
    wrong = ps.wrong_expected(b)
    assert b.n == 256 and len(set(b.expected)) == 256
    for i, (w, t) in enumerate(zip(wrong, b.tops)):
        diff = int.from_bytes(w, "little") ^ int.from_bytes(t, "little")
        assert diff == 1 << i  # bit i of the row as a 256-bit little-endian number: byte i // 8, bit i % 8
    assert {i // 32 for i in range(256)} == set(range(8))  # every word of the compare, every bit of each


@pytest.mark.parametrize("zero_expected", [False, True])
def test_bad_descriptors(zero_expected):
    a, b = ps.bad_batch(0xFF, zero_expected), ps.bad_batch(0x5A, zero_expected)
    assert a.n == b.n == 300 and a.proofs == b.proofs and a.tops == b.tops and a.expected == b.expected
    assert _in_bounds(a), "no descriptor points outside the tensor"
    assert {p[3] for i, p in enumerate(a.proofs) if i in ps.BAD_AT} == {0, 3, 768, 1024, 4, 2}
    assert {p[4] for i, p in enumerate(a.proofs) if i in ps.BAD_AT} >= {65, 255}
    assert {i // ps.WAVE for i in ps.BAD_AT} == {0, 1, 2, 3, 4} and {0, 63, 64, 255, 256, 299} <= set(ps.BAD_AT)
    guard = {k for k, (x, y) in enumerate(zip(a.rows, b.rows)) if x != y}
    assert len(guard) == ps.BAD_GUARD and guard == set(range(min(guard), min(guard) + ps.BAD_GUARD))
    for i, (pos, row, e, span, uncles) in enumerate(a.proofs):
        rows = set(range(row, row + span + uncles))
        if i in ps.BAD_AT:
            assert rows <= guard and a.tops[i] == bytes(32)
            assert a.expected[e] == bytes(32) if zero_expected else a.expected[e] != bytes(32)
        else:
            assert not rows & guard and a.expected[e] == a.tops[i]


def test_far_rows():
    block, proofs, expected, tops = ps.far_proofs()
    assert ps.FAR_BASE * 32 == 1 << 32 and len(block) == 2049
    assert [(p[1] - ps.FAR_BASE, p[3], p[4]) for p in proofs] == [(-1, 1, 2), (0, 2, 64), (600, 512, 3), (1500, 64, 0)]
    assert all(p[1] + p[3] + p[4] <= ps.FAR_ROWS for p in proofs) and expected == tops
    assert proofs[0][1] * 32 < 1 << 32 <= (proofs[0][1] + 1) * 32  # the span row before the line, the uncles behind
