"""The item list and the stored-tile predicate of the symmetric walk from the unpopular side (CoocArgs::half == 2, fy_cooc.hpp:
cooc_rect_item_index, cooc_item_count, cooc_tile_stored), restated in Python: the closed form numbers the (row, chunk) items of a launch
0 ... count - 1 without a gap, rows ascending and chunks ascending inside a row, and of every off-diagonal 256 x 256 tile exactly one of
(B, T) and (T, B) is stored -- the other is what the mirror pass writes."""
import numpy as np
import pytest

SHAPES = [(700, 256), (700, 512), (2400, 768), (59047, 19712)]


def item_index(row, ch, CH):
    c = row // CH
    return CH * (c * (c + 1) // 2) + (row - c * CH) * (c + 1) + ch


def item_count(Ic, CH):
    return item_index(Ic - 1, (Ic - 1) // CH, CH) + 1


def tile_stored(B, T, bpc):
    cB, cT = B // bpc, T // bpc
    return T > B if cT == cB else cT < cB


@pytest.mark.parametrize("Ic,CH", SHAPES)
def test_item_index_is_a_bijection(Ic, CH):
    rows = np.arange(Ic, dtype=np.int64)
    own = rows // CH
    n_items = int((own + 1).sum())                       # a row of chunk c has items for the chunks 0 ... c
    assert item_count(Ic, CH) == n_items
    row_of = np.repeat(rows, own + 1)
    first = np.cumsum(own + 1) - (own + 1)
    ch_of = np.arange(n_items, dtype=np.int64) - np.repeat(first, own + 1)
    assert np.all(ch_of <= row_of // CH) and np.all(ch_of >= 0)
    c = row_of // CH
    at = CH * (c * (c + 1) // 2) + (row_of - c * CH) * (c + 1) + ch_of
    assert np.array_equal(at, np.arange(n_items))       # rows ascending, chunks ascending inside a row, no gap
    for row, ch in ((0, 0), (CH - 1, 0), (CH, 0), (CH, 1), (Ic - 1, (Ic - 1) // CH)):
        assert item_index(row, ch, CH) == int(at[(row_of == row) & (ch_of == ch)][0])


@pytest.mark.parametrize("Ic,CH", SHAPES)
def test_every_off_diagonal_tile_is_stored_once(Ic, CH):
    nblk, bpc = -(-Ic // 256), CH // 256
    B, T = np.meshgrid(np.arange(nblk), np.arange(nblk), indexing="ij")
    cB, cT = B // bpc, T // bpc
    stored = np.where(cB == cT, T > B, cT < cB)
    off = B != T
    assert np.all(stored[off] ^ stored.T[off])           # exactly one of a tile and its transpose
    assert not stored[~off].any()                        # the diagonal blocks are k_mirror_diag's
    # what the epilogue stores: a row of block B keeps its own chunk behind its diagonal block and the whole chunks in front of it
    for b in (0, bpc - 1, bpc, nblk - 1):
        want = [t for t in range(nblk) if (t // bpc == b // bpc and t > b) or t // bpc < b // bpc]
        assert [t for t in range(nblk) if tile_stored(b, t, bpc)] == want
    assert not stored[0, bpc:].any() and stored[nblk - 1, :((nblk - 1) // bpc) * bpc].all()
