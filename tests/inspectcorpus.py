"""The streams the inspection tests run on, and their expected rows (tests/lacinspect.py, computed once per process).

  pinned()        the streams of tests/golden/decode_wav.json: the committed fixtures, their version-2 rewrites and the
                  257- and 4097-frame splices
  small()         the files of tests/golden/small/
  narrow(oracle)  the streams of narrowrecipes.py, encoded by the oracle
  grammar()       every case of lacgrammar.ALL_NAMES, with its declared status
  cuts(lac)       a version-3 stream cut at every kind of place behind its table
  expected(lac)   lacinspect.inspect_stream, memoised; seen(lac): what that walk met
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import lacgrammar
import lacinspect
import lacstreams
import narrowrecipes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_expected, _seen = {}, {}


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def pinned():
    with open(os.path.join(GOLDEN, "decode_wav.json")) as f:
        ents = json.load(f)
    return tuple((e["name"], lacstreams.from_recipe(e["source"], _fixture)) for e in ents)


@functools.lru_cache(maxsize=None)
def small():
    with open(os.path.join(GOLDEN, "small", "index.json")) as f:
        ents = json.load(f)
    return tuple((e["name"], _fixture("small/%s.lac" % e["name"])) for e in ents)


@functools.lru_cache(maxsize=None)
def narrow(oracle):
    out = []
    for k, (name, depth, left, right) in enumerate(narrowrecipes.streams() + narrowrecipes.stereo_streams()):
        out.append((name, oracle.encode(left, right, 48000, depth, (2, 1, 0)[k % 3], threads=8)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def grammar():
    """((name, lac, declared status, bad block), ...)."""
    out = []
    for name in lacgrammar.ALL_NAMES:
        s = lacgrammar.build(name)
        out.append((name, s.lac, s.status, s.bad_block))
    return tuple(out)


def cuts(lac):
    """The stream cut inside its last block, at a block border, one byte into the payload and right behind the table."""
    nb, ent, payload = lacstreams._table(lac)
    head = len(lac) - len(payload)
    places = {head, head + 1, len(lac) - 1, len(lac) - ent[-1][1], len(lac) - ent[-1][1] + 1}
    if nb > 1:
        places |= {head + ent[0][1], head + ent[0][1] - 1}
    return [lac[:at] for at in sorted(places) if head <= at < len(lac)]


def expected(lac):
    key = bytes(lac)
    if key not in _expected:
        lacinspect.SEEN.clear()
        _expected[key] = lacinspect.inspect_stream(key)
        _seen[key] = frozenset(lacinspect.SEEN)
    return _expected[key]


def seen(lac):
    """What the walk of this stream met (lacinspect.SEEN)."""
    expected(lac)
    return _seen[bytes(lac)]


def stereo_flag(lac):
    return lac[3] == 2 and lac[4] == 2


def mid_side(left, right):
    """The forward transform of the format (ref lac/encoder.cpp): side = left - right, mid = left - ((side + (side & 1)) >> 1)."""
    l, r = np.asarray(left, np.int64), np.asarray(right, np.int64)
    s = l - r
    return (l - ((s + (s & 1)) >> 1)).astype(np.int32), s.astype(np.int32)
