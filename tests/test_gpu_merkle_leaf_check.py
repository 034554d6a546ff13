"""GPU: merkle_leaf_check_kernel alone, through device.merkle_leaf_check, on
random rows against a numpy model: the bitmap's words (several pieces per wave,
one word, many words, more words per piece than the group needs), the shadow
rows and the copy-out, each mode alone and together.  Every output tensor is
pre-filled and larger than what the kernel may write; what it must not touch
must come back as it was.  Nothing is hashed here: the kernel compares rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (log2_width, n, row0, extra words per piece)
CASES = [
    (0, 1, 0, 0),      # one row
    (0, 67, 5, 0),     # 64 pieces per wave, the second wave partial
    (2, 19, 4, 0),     # 16 pieces per wave, n no multiple of 16
    (2, 19, 0, 1),     # ... under a wider call: wpp 2
    (5, 3, 32, 0),     # two pieces per wave, the last wave half empty
    (5, 9, 1, 3),      # 288 rows: a partial second workgroup
    (6, 1, 0, 0),      # exactly one word
    (6, 5, 64, 1),     # 320 rows: a partial second workgroup, wpp 2
    (7, 3, 128, 0),    # two words per piece
    (7, 2, 3, 2),      # ... of four
    (11, 1, 0, 0),     # a wide piece: 32 words, 8 workgroups
    (11, 2, 2048, 0),
]


def _blocks(K, n, rng):
    W = 1 << K
    want = [W, 1, max(1, W - 1)] + ([65, 64, 63] if K >= 7 else [])
    while len(want) < n:
        want.append(int(rng.integers(1, W + 1)))
    return np.array(want[:n], dtype=np.int32)


class Case:
    """The window, the stored table and what the kernel must make of them."""

    def __init__(self, K, n, row0, extra, seed):
        rng = np.random.default_rng(seed)
        W = 1 << K
        self.K, self.n, self.row0 = K, n, row0
        self.need = max(1, W // 64)
        self.wpp = self.need + extra
        self.blocks = _blocks(K, n, rng)
        self.base = 3  # the table has rows in front of the pieces' and behind them
        self.first = (self.base + np.concatenate([[0], np.cumsum(self.blocks)[:-1]])).astype(np.int32)
        self.T = int(self.base + self.blocks.sum() + 2)
        self.R = row0 + n * W + 7
        self.window = rng.integers(0, 256, (self.R, 32), dtype=np.uint8)  # dead slots: garbage that differs
        # the stored table: the window's live rows, then the damage
        self.stored = rng.integers(0, 256, (self.T, 32), dtype=np.uint8)
        self.compact = np.full((self.T, 32), 0xFF, dtype=np.uint8)  # what copy-out must give
        for k in range(n):
            rows = self.window[row0 + k * W:row0 + k * W + self.blocks[k]]
            self.stored[self.first[k]:self.first[k] + self.blocks[k]] = rows
            self.compact[self.first[k]:self.first[k] + self.blocks[k]] = rows
        self.bad_slots = {}
        for k in range(n):
            nb = int(self.blocks[k])
            slots = {s for s in (0, 63, 64, nb - 1) if s < nb} if k % 3 != 1 else set()
            if k % 4 == 3:
                slots |= {int(s) for s in rng.integers(0, nb, 3)}
            self.bad_slots[k] = sorted(slots)
            for s in slots:
                self.stored[self.first[k] + s, int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        # the model
        self.fill = 0x5555555555555555
        self.words = np.full(n * self.wpp + 2, self.fill, dtype=np.uint64)
        for k in range(n):
            for w in range(self.need):
                self.words[k * self.wpp + w] = sum(1 << (s - 64 * w) for s in self.bad_slots[k] if s // 64 == w)
        self.shadow = np.full((self.R, 32), 0xEE, dtype=np.uint8)
        for k in range(n):
            at = row0 + k * W
            self.shadow[at:at + W] = 0
            self.shadow[at:at + self.blocks[k]] = self.stored[self.first[k]:self.first[k] + self.blocks[k]]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "K%d-n%d-row%d-x%d" % c)
def case(request):
    return Case(*request.param, seed=sum(request.param) + 1)


def _run(gpu, c, check, shadow, copy):
    import torch

    from vortex_amd import device as vdev

    t = lambda a: torch.from_numpy(a.copy()).to(gpu)  # noqa: E731
    window, first, blocks = t(c.window), t(c.first), t(c.blocks)
    bad = torch.from_numpy(np.full(c.n * c.wpp + 2, c.fill, dtype=np.uint64).view(np.int64)).to(gpu) if check else None
    sh = torch.full((c.R, 32), 0xEE, dtype=torch.uint8, device=gpu) if shadow else None
    out = torch.full((c.T, 32), 0xFF, dtype=torch.uint8, device=gpu) if copy else None
    got = vdev.merkle_leaf_check(window, c.row0, c.n, c.K, first, blocks,
                                 expected_leaves=t(c.stored) if check else None, bad=bad, wpp=c.wpp, shadow=sh,
                                 leaves_out=out)
    torch.cuda.synchronize()
    assert (window.cpu().numpy() == c.window).all(), "the kernel wrote to its window"
    return [x.cpu().numpy() if x is not None else None for x in got]


def test_check_shadow_and_copy_out_together(gpu, built, case):
    bad, shadow, out = _run(gpu, case, True, True, True)
    assert (bad.view(np.uint64) == case.words).all(), (bad.view(np.uint64), case.words)
    assert (shadow == case.shadow).all()
    assert (out == case.compact).all()


def test_check_alone(gpu, built, case):
    bad, shadow, out = _run(gpu, case, True, False, False)
    assert shadow is None and out is None
    assert (bad.view(np.uint64) == case.words).all()


def test_check_with_shadow(gpu, built, case):
    bad, shadow, _ = _run(gpu, case, True, True, False)
    assert (bad.view(np.uint64) == case.words).all()
    assert (shadow == case.shadow).all()


def test_copy_out_alone(gpu, built, case):
    bad, shadow, out = _run(gpu, case, False, False, True)
    assert bad is None and shadow is None
    assert (out == case.compact).all()


def test_the_shadow_reduces_like_the_stored_rows(gpu, built):
    """What the files call does with the shadow: the node kernels over it give
    the root of the stored rows, zeros in the dead slots."""
    import hashlib

    import torch

    from vortex_amd import device as vdev

    c = Case(3, 5, 8, 0, seed=99)
    _, shadow, _ = _run(gpu, c, True, True, False)
    roots, _ = vdev.merkle_nodes(torch.from_numpy(shadow[c.row0:c.row0 + (c.n << c.K)].copy()).to(gpu), c.n, c.K)
    torch.cuda.synchronize()
    for k in range(c.n):
        rows = [bytes(c.stored[c.first[k] + s]) if s < c.blocks[k] else bytes(32) for s in range(1 << c.K)]
        while len(rows) > 1:
            rows = [hashlib.sha256(rows[j] + rows[j + 1]).digest() for j in range(0, len(rows), 2)]
        assert bytes(roots[k].cpu().numpy()) == rows[0]


def test_device_metadata_is_validated(gpu, built):
    import torch

    from vortex_amd import device as vdev

    c = Case(2, 4, 0, 0, seed=5)
    t = lambda a, **kw: torch.from_numpy(a.copy()).to(gpu)  # noqa: E731
    window, first, blocks, stored = t(c.window), t(c.first), t(c.blocks), t(c.stored)
    for bad_blocks in ([0, 1, 1, 1], [5, 1, 1, 1]):
        with pytest.raises(ValueError, match="blocks"):
            vdev.merkle_leaf_check(window, 0, 4, 2, first, torch.tensor(bad_blocks, dtype=torch.int32, device=gpu),
                                   expected_leaves=stored)
    with pytest.raises(ValueError, match="table"):
        vdev.merkle_leaf_check(window, 0, 4, 2, first + c.T, blocks, expected_leaves=stored)
    with pytest.raises(ValueError, match="window"):
        vdev.merkle_leaf_check(window, c.R, 4, 2, first, blocks, expected_leaves=stored)
    with pytest.raises(ValueError, match="wpp"):
        vdev.merkle_leaf_check(window, 0, 4, 2, first, blocks, expected_leaves=stored, wpp=0)
    with pytest.raises(ValueError, match="neither"):
        vdev.merkle_leaf_check(window, 0, 4, 2, first, blocks)
    with pytest.raises(ValueError, match="need expected_leaves"):
        vdev.merkle_leaf_check(window, 0, 4, 2, first, blocks, shadow=torch.zeros_like(window), leaves_out=stored)
