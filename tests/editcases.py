"""Sources and expectations of the transcode tests (lacx_transcode_batch).  The sources are minted from frozen seeds
through the oracle, once per process; the expectation of an output is the oracle as a pipeline: oracleshim.decode of every
source, sliced, concatenated and transformed in numpy, then oracleshim.encode of the result.

  sources()                       {name: Source(lac, left, right, rate, depth)}
  expected(segments, ...)         Expected(lac, crc, frames, blocks, channels, depth, rate) of one output
  apply(left, right, depth, op, to_depth)   the channel operation and the depth change in numpy -> (left, right, depth, error)
"""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np

import __graft_entry__ as ge
import lacinspect
import lacstreams
import oracleshim
import wavutil

Source = namedtuple("Source", "lac left right rate depth")
Expected = namedtuple("Expected", "lac crc frames blocks channels depth rate")
KEEP, LEFT, RIGHT, FOLD, SWAP, DUAL = range(6)
OPS = ("keep", "left", "right", "fold", "swap", "dual")
FRAMES = 40000  # blocks of 16384, 16384 and 7232 frames


def _mint(left, right, rate, depth, mode):
    lac = oracleshim.encode(left, right, rate, depth, mode)
    l2, r2, _ = oracleshim.decode(lac)  # the expectation starts from what the oracle decodes
    return Source(lac, l2, r2, rate, depth)


def block_ms_flags(lac):
    """The mid/side flag of every block of a version-3 stream in stereo mode 2: the first byte of its payload."""
    version, channels, mode, _, _, table = lacinspect.head(lac)
    assert version == 3 and channels == 2 and mode == 2
    at, flags = 14 + 8 * len(table), []
    for _, nbytes in table:
        flags.append(lac[at])
        at += nbytes
    return flags


@functools.lru_cache(maxsize=None)
def sources():
    synth = ge.load_pkg().synth
    # stereo 16 / 48k: a narrow block (mid/side wins), a block of independent noise (left/right wins), a narrow rest
    a = synth.synth_pcm(16384, 2, 16, 48000, seed=101, kind="music", stereo="narrow")
    b = synth.synth_pcm(16384, 2, 16, 48000, seed=102, kind="noise", stereo="independent", start=16384)
    c = synth.synth_pcm(FRAMES - 32768, 2, 16, 48000, seed=103, kind="music", stereo="narrow", start=32768)
    left, right = np.concatenate([a[0], b[0], c[0]]), np.concatenate([a[1], b[1], c[1]])
    out = {"st16_lr": _mint(left, right, 48000, 16, 0), "st16_ms": _mint(left, right, 48000, 16, 1),
           "st16_auto": _mint(left, right, 48000, 16, 2)}
    out["st16_auto_ms"] = block_ms_flags(out["st16_auto"].lac)
    other = synth.synth_pcm(20000, 2, 16, 48000, seed=104, kind="walk", stereo="wide")
    out["st16_other"] = _mint(other[0], other[1], 48000, 16, 2)
    mono = synth.synth_pcm(20000, 1, 24, 96000, seed=105, kind="music")
    out["mono24"] = _mint(mono[0], None, 96000, 24, 0)
    n16 = synth.synth_pcm(20000, 2, 16, 48000, seed=106, kind="music", stereo="wide")
    out["st24_narrowable"] = _mint(n16[0] * 256, n16[1] * 256, 48000, 24, 2)
    dm = synth.synth_pcm(20000, 2, 16, 48000, seed=107, kind="music", stereo="identical")
    out["dual_mono"] = _mint(dm[0], dm[1], 48000, 16, 2)
    dm24 = synth.synth_pcm(20000, 2, 16, 48000, seed=108, kind="walk", stereo="identical")
    out["dual_mono24_narrowable"] = _mint(dm24[0] * 256, dm24[1] * 256, 48000, 24, 2)
    # 24-bit stereo that is not narrowable, and only on the right: left all multiples of 256, right from frame 5 on not
    ro = synth.synth_pcm(3000, 2, 16, 48000, seed=109, kind="music", stereo="wide")
    out["st24_right_odd"] = _mint(ro[0] * 256, ro[1] * 256 + (np.arange(3000) >= 5), 48000, 24, 2)
    s = out["st16_auto"]
    out["st16_v2"] = Source(lacstreams.to_v2(s.lac), s.left, s.right, s.rate, s.depth)
    return out


def apply(left, right, depth, op, to_depth):
    """The channel operation, then the depth change -> (left, right, depth, error text or None): the first violation in
    frame order, within a frame the channel operation first, then left before right."""
    bad = []  # (frame, rank, text)
    if op == FOLD:
        d = np.flatnonzero(left != right)
        if d.size:
            f = int(d[0])
            bad.append((f, 0, f"[transcode-error] frame {f}: left {int(left[f])} and right {int(right[f])} differ"))
    if op in (LEFT, FOLD):
        right = None
    elif op == RIGHT:
        left, right = right, None
    elif op == SWAP:
        left, right = right, left
    elif op == DUAL:
        right = left.copy()
    to_depth = to_depth or depth
    if depth == 24 and to_depth == 16:
        for rank, (name, ch) in enumerate((("left", left), ("right", right)), 1):
            if ch is None:
                continue
            d = np.flatnonzero(ch & 0xFF)
            if d.size:
                f = int(d[0])
                bad.append((f, rank, f"[transcode-error] frame {f} {name} sample {int(ch[f])} is not a multiple of 256"))
        left, right = left >> 8, None if right is None else right >> 8
    elif depth == 16 and to_depth == 24:
        left, right = left << 8, None if right is None else right << 8
    return left, right, to_depth, (min(bad)[2] if bad else None)


def edited(segments, bit_depth=0, op=KEEP):
    """segments: [(source name or Source, start, frames or None)] -> (left, right, rate, depth, error)."""
    src = sources()
    parts = []
    for name, start, frames in segments:
        s = src[name] if isinstance(name, str) else name
        end = s.left.size if frames is None else start + frames
        parts.append((s.left[start:end], None if s.right is None else s.right[start:end], s))
    left = np.concatenate([p[0] for p in parts])
    right = None if parts[0][1] is None else np.concatenate([p[1] for p in parts])
    s0 = parts[0][2]
    l, r, depth, error = apply(left, right, s0.depth, op, bit_depth)
    return l, r, s0.rate, depth, error


def expected(segments, bit_depth=0, op=KEEP, stereo_mode=2, zero_run=True, partitioning=True) -> Expected:
    l, r, rate, depth, error = edited(segments, bit_depth, op)
    assert error is None, error
    lac = oracleshim.encode(l, r, rate, depth, stereo_mode if r is not None else 0, zero_run, partitioning)
    return Expected(lac, zlib.crc32(wavutil.pcm_bytes(l, r, depth)), int(l.size), (int(l.size) + 16383) // 16384,
                    1 if r is None else 2, depth, rate)
