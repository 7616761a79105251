"""Host: the sentence-packing plan of the BERT text path (mec_text_pack_plan, include/mec.h): first-fit
decreasing over 128-slot rows, specified exactly -- samples by length descending (ties by ascending
index), each into the lowest-numbered row with room at that row's fill, a new row when none has room --
so the numpy mirror below reproduces it entry for entry. No GPU: the plan is host code, and the
argument errors of mec_text_fwd_packed are raised before any device call."""
import ctypes

import numpy as np
import pytest

from mec import _lib, synthetic as syn

IP = ctypes.POINTER(ctypes.c_int32)


def _plan(lens):
    lens = np.ascontiguousarray(lens, np.int32)
    row, off = np.full(lens.size, -7, np.int32), np.full(lens.size, -7, np.int32)
    bp = _lib.load().mec_text_pack_plan(lens.ctypes.data_as(IP), int(lens.size), row.ctypes.data_as(IP),
                                        off.ctypes.data_as(IP))
    return bp, row, off


def _mirror(lens):
    """First-fit decreasing, as include/mec.h states it."""
    lens = np.asarray(lens, np.int64)
    row, off, fill = np.zeros(lens.size, np.int32), np.zeros(lens.size, np.int32), []
    for i in np.argsort(-lens, kind='stable'):
        r = next((r for r, f in enumerate(fill) if 128 - f >= lens[i]), len(fill))
        if r == len(fill):
            fill.append(0)
        row[i], off[i] = r, fill[r]
        fill[r] += lens[i]
    return len(fill), row, off


@pytest.mark.parametrize('lens,bp', [([8] * 16, 1), ([8] * 17, 2), ([64] * 4, 2), ([65] * 4, 4),
                                     ([128, 8, 60, 60, 9], 3)])
def test_hand_checked_row_counts(lens, bp):
    got, row, off = _plan(lens)
    assert got == bp
    assert _mirror(lens)[0] == bp


def test_hand_checked_rows_and_offsets():
    bp, row, off = _plan([128, 8, 60, 60, 9])
    assert bp == 3
    assert row.tolist() == [0, 1, 1, 1, 2]
    assert off.tolist() == [0, 120, 0, 60, 0]


@pytest.mark.parametrize('B', [1, 5, 64, 257])
def test_plan_equals_numpy_mirror_and_is_a_valid_packing(B):
    _, mask = syn.text_inputs(B, ragged=True)
    lens = mask.sum(1).astype(np.int32)
    bp, row, off = _plan(lens)
    mbp, mrow, moff = _mirror(lens)
    assert bp == mbp
    np.testing.assert_array_equal(row, mrow)
    np.testing.assert_array_equal(off, moff)
    # every sample placed once, inside a row; spans of a row disjoint; Bp between the volume bound and B
    assert ((row >= 0) & (row < bp)).all() and (off >= 0).all() and (off + lens <= 128).all()
    used = np.zeros((bp, 128), np.int32)
    for r, o, n in zip(row, off, lens):
        used[r, o:o + n] += 1
    assert used.max() == 1 and used.sum() == lens.sum()
    assert (used.sum(1) > 0).all()  # no empty row
    assert -(-int(lens.sum()) // 128) <= bp <= B


def test_empty_batch_returns_zero():
    lib = _lib.load()
    assert lib.mec_text_pack_plan(None, 0, None, None) == 0
    assert _plan(np.zeros(0, np.int32))[0] == 0


@pytest.mark.parametrize('bad', [0, 129, -3])
def test_length_outside_range_is_an_error(bad):
    bp, _, _ = _plan([5, bad, 7])
    assert bp == -1
    assert b'[1,128]' in _lib.load().mec_last_error()


def test_null_pointers_and_negative_count_are_errors():
    lib = _lib.load()
    a = np.array([4, 5], np.int32)
    p = a.ctypes.data_as(IP)
    for args in ((None, 2, p, p), (p, 2, None, p), (p, 2, p, None)):
        assert lib.mec_text_pack_plan(*args) == -1
        assert b'[1,128]' in lib.mec_last_error()
    assert lib.mec_text_pack_plan(p, -1, p, p) == -1


def test_fwd_packed_null_model_without_gpu():
    lib = _lib.load()
    assert lib.mec_text_fwd_packed(None, None, None, None, None, 4, 2, None, None, None, None) == -1
    assert b'null model' in lib.mec_last_error()
