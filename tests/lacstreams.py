"""Container-level rewrites of .lac streams for the decode tests (no codec work: block payloads are moved, never
re-encoded).  The layout (ref src/codec/lac/decoder.cpp:84-219): a 10-byte frame header, a big-endian block count,
then per block its frame count and -- version 3 only -- its compressed size, then the block payloads back to back.

  to_v2(lac)            the legacy version-2 container of the same blocks (no compressed sizes)
  take_blocks(lac, a, b) blocks [a, b) of a version-3 stream as a stream of their own (blocks are independent)
  splice(a, b)          two version-3 streams with equal frame headers as one: tables and payloads concatenated, so
                        that a's final block becomes a NON-final block of whatever length it had (257, 4097, ...)
"""
import struct


def _table(lac: bytes):
    nb = struct.unpack(">I", lac[10:14])[0]
    ent = [struct.unpack(">II", lac[14 + 8 * b:22 + 8 * b]) for b in range(nb)]
    return nb, ent, lac[14 + 8 * nb:]


def _build(header: bytes, ent, payload: bytes) -> bytes:
    return header + struct.pack(">I", len(ent)) + b"".join(struct.pack(">II", n, s) for n, s in ent) + payload


def to_v2(lac: bytes) -> bytes:
    assert lac[2] == 3
    nb, ent, payload = _table(lac)
    return lac[:2] + bytes([2]) + lac[3:14] + b"".join(struct.pack(">I", n) for n, _ in ent) + payload


def block_frames(lac: bytes):
    """Frame counts of the blocks of a version-3 stream."""
    return [n for n, _ in _table(lac)[1]]


def take_blocks(lac: bytes, start: int, end: int) -> bytes:
    assert lac[2] == 3
    nb, ent, payload = _table(lac)
    assert 0 <= start < end <= nb
    off = sum(s for _, s in ent[:start])
    size = sum(s for _, s in ent[start:end])
    return _build(lac[:10], ent[start:end], payload[off:off + size])


def splice(a: bytes, b: bytes) -> bytes:
    assert a[:10] == b[:10] and a[2] == 3, "splice needs equal version-3 frame headers"
    _, ea, pa = _table(a)
    _, eb, pb = _table(b)
    return _build(a[:10], ea + eb, pa + pb)


def frame_ranges(lac: bytes, start: int, end: int):
    """(first frame, end frame) of blocks [start, end) of a version-3 stream, within that stream."""
    fr = block_frames(lac)
    return sum(fr[:start]), sum(fr[:end])


def from_recipe(recipe, read):
    """The stream a decode_wav.json `source` describes; read(name) -> bytes of a committed fixture."""
    if "file" in recipe:
        lac = read(recipe["file"])
        if "blocks" in recipe:
            lac = take_blocks(lac, *recipe["blocks"])
        return lac
    if "v2" in recipe:
        return to_v2(from_recipe(recipe["v2"], read))
    if "splice" in recipe:
        parts = [from_recipe(r, read) for r in recipe["splice"]]
        out = parts[0]
        for p in parts[1:]:
            out = splice(out, p)
        return out
    raise ValueError(f"unknown recipe {recipe!r}")
