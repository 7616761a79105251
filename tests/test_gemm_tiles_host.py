"""Which tile ids the GEMM option keys accept, swept over every value (no GPU: mec_set_option only sets
the process defaults). The id lists here are the test's own statement of the catalogue
(csrc/gemm_tiles.h), written out, not read from the library."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'multimodal-emotion-classification_amd'))

from mec import _lib  # noqa: E402

GLDS_TILES = [64, 128, 256, 1128, 1064, 10064, 10128, 10256, 11128, 11064, 20256, 30256, 20128, 40256, 41256,
              50128, 60128, 50256]
X3I_TILES = [70256, 70128, 71128, 71064, 70064, 72128]
F32_TILES = [1, 2, 3, 4, 5, 6, 7, 8]
TAGS = range(1, 15)          # the launch classes a per-tag key addresses (tag * 100000 + id)
TAG_DEFAULTS = {b'gemm_bn_tag': {3: 11128}, b'gemm_x3_tag': {4: 70256, 5: 72128}, b'gemm_f32_tag': {4: 8}}


def accepted(lib, key, values):
    return {v for v in values if lib.mec_set_option(key, v) == 0}


def test_tile_option_keys_accept_exactly_the_catalogue():
    lib = _lib.load()
    assert len(GLDS_TILES) + len(X3I_TILES) == 24
    tiles = {0} | set(GLDS_TILES) | set(X3I_TILES)
    try:
        assert accepted(lib, b'gemm_bn', range(-1, 100001)) == tiles
        assert accepted(lib, b'gemm_f32_tile', range(-1, 100001)) == {0} | set(F32_TILES)
        # per-tag keys: every id value 0 .. 99999 on every tag for gemm_bn_tag and on the first and last tag for
        # the other two; on the tags between, every catalogued id of either engine and the values next to 0 .. 8
        every = range(100000)
        known = sorted(tiles | set(range(10)))
        for t in TAGS:
            sweep = every if t in (1, 14) else known
            assert accepted(lib, b'gemm_bn_tag', (t * 100000 + v for v in every)) == {t * 100000 + v for v in tiles}, t
            assert accepted(lib, b'gemm_x3_tag', (t * 100000 + v for v in sweep)) == \
                {t * 100000 + v for v in [0] + X3I_TILES}, t
            assert accepted(lib, b'gemm_f32_tag', (t * 100000 + v for v in sweep)) == \
                {t * 100000 + v for v in [0] + F32_TILES}, t
        for t in (0, 15):  # no such launch class
            for key in TAG_DEFAULTS:
                sweep = every if key == b'gemm_bn_tag' else known
                assert accepted(lib, key, (t * 100000 + v for v in sweep)) == set(), (key, t)
        for key in TAG_DEFAULTS:
            assert accepted(lib, key, [-1, -70256, 16 * 100000, 16 * 100000 + 8, 2 ** 31 - 1]) == set(), key
    finally:  # the defaults
        lib.mec_set_option(b'gemm_bn', 0)
        lib.mec_set_option(b'gemm_f32_tile', 0)
        for key, pins in TAG_DEFAULTS.items():
            for t in TAGS:
                lib.mec_set_option(key, t * 100000 + pins.get(t, 0))
