"""A seeded, deterministic corpus of damaged .lac streams: what nobody designed.

Every mutant is (base name, mutator family, parameters) -> bytes; the generator needs no built library (the one place
that does -- finding the second channel block of a stereo block -- takes a function from the caller).  All mutators leave
the frame header and the block table such that lacx.stream_parse still accepts the stream; the tests assert that.

  bases(block_end)    name -> stream: the committed fixtures, lacgrammar's valid cases (one per family at least) and
                      version-2 rewrites of some of them
  corpus(block_end)   [Mutant]: name, base, family, lac
  FAMILIES            hdrflip  every single-bit flip in the header region of every channel block of the fixtures and small bases
                               (flag byte .. end of the partition table) and in the first / last 8 bytes of every block
                      flip     1-4 random bit flips anywhere in the payload
                      run      a run of 1-64 bytes of 0xFF / 0x00 / 0xAA / random bytes: at a random place, ending at
                               a block's last byte, ending at the stream's last byte (a long unary run into the pad)
                      table    1-40 bytes moved between two neighbouring table entries, payload untouched
                      transplant  two blocks' payloads swapped, or one copied over another, the table's sizes fixed
                      trunc    a block's payload cut by 1-30 bytes or extended by zero / 0xFF bytes, the table fixed
                      escape   the 32 bits behind a zero-run escape tag, and a partition's 5-bit k, at their extremes
  unchanged_blocks(base, lac)  the blocks of a version-3 mutant that are byte-identical to the base's at the same place
"""
from __future__ import annotations

import glob
import os
import random
import struct
from collections import namedtuple

import lacgrammar as g
import lacstreams

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILIES = ("hdrflip", "flip", "run", "table", "transplant", "trunc", "escape")
Mutant = namedtuple("Mutant", "name base family lac")

# lacgrammar's valid cases by family: LPC order above 12, stateful / stateless zero-run, bin, static, partition order 8,
# a 5000-bit unary run, mid/side at 16 and 24 bit, and the rest of the grammar in small blocks
GRAMMAR_BASES = ["lpc_o13_min", "lpc_o20_mid", "lpc_o32_min", "lpc_o7_mid", "zero_run_runs_stateful", "zero_run_runs_stateless",
                 "zero_run_escapes", "zero_run_to_exact_end_stateful", "bin_all_tags", "bin_stateful_small_values",
                 "rice_static_k0", "rice_static_k29", "rice_adaptive_k0", "partition_p8_smallest_n", "partition_p1_smallest_n",
                 "unary_5000", "unary_64", "unary_terminator_last_bit", "stereo_mode_1_16bit", "stereo_mode_1_24bit",
                 "stereo_side_parities", "fir_n3", "fixed4_n3", "stateful_rice_loud_then_quiet", "sweep_03", "sweep_11",
                 "wave_mix_rotating_families"]
V2_BASES = ["small/n257_st16_ms", "small/n2400_mono16_selftest", "decode_wav/st16_lr_3blk", "lpc_o13_min", "unary_5000",
            "zero_run_runs_stateless", "bin_all_tags", "stereo_mode_1_24bit", "sweep_03", "equal_blocks_mono"]
SMALL_FRAMES, FEW_BLOCKS = 6000, 3   # bases of at most this many frames, or blocks, get the exhaustive flips: every
# fixture under golden/ (a 16384-frame block's header included) and every grammar base but the long many-block ones


def _rng(name):
    return random.Random("lacmutate:" + name)


def table(lac):
    """(version, [(frames, bytes)], head): the bytes of a version-2 stream's blocks are unknown (None)."""
    nb = struct.unpack(">I", lac[10:14])[0]
    if lac[2] == 3:
        ent = [struct.unpack(">II", lac[14 + 8 * b:22 + 8 * b]) for b in range(nb)]
        return 3, ent, 14 + 8 * nb
    return 2, [(struct.unpack(">I", lac[14 + 4 * b:18 + 4 * b])[0], None) for b in range(nb)], 14 + 4 * nb


def _rebuild(lac, ent, payloads):
    return lacstreams._build(lac[:10], [(n, len(p)) for (n, _), p in zip(ent, payloads)], b"".join(payloads))


def _payloads(lac):
    _, ent, head = table(lac)
    out, off = [], head
    for _, size in ent:
        out.append(lac[off:off + size])
        off += size
    return ent, out


def header_extent(cb: bytes, n: int) -> int:
    """Bytes of a (valid) channel block that hold its header: type, order, the coefficient list, the control byte and
    the partition table (ref block/decoder.cpp:64-140), walked from the bytes."""
    ptype, order = cb[0], cb[1]
    bits = 16 + (16 * order if ptype == 2 else 0)
    p = cb[bits // 8] & 0x0F
    parts = (1 << p) if (p and (n >> p)) else 1
    return (bits + 8 + 7 * parts + 7) // 8


def header_regions(lac, block_end):
    """Per block of a version-3 stream: the byte ranges (within the file) of the flag byte and of each channel block's
    header.  block_end(bytes, n) -> the length of the channel block at the start of `bytes`."""
    _, ent, head = table(lac)
    channels, flagged = lac[3], lac[3] == 2 and lac[4] == 2
    out, off = [], head
    for n, size in ent:
        pay = lac[off:off + size]
        at = 1 if flagged else 0
        regions = [(off, off + at)] if flagged else []
        for c in range(channels):
            regions.append((off + at, off + at + min(header_extent(pay[at:], n), size - at)))
            if c + 1 < channels:
                at += block_end(pay[at:], n)
        out.append(regions)
        off += size
    return out


def equal_blocks(name, channels):
    """Eight blocks of 512 frames (a copied payload decodes where it lands), every token family."""
    rng = g._rng("lacmutate:" + name)
    blocks = [g.Block([g.random_channel_block(rng, 512, 16, side=(c == 1), family=g.FAMILIES[(i + c) % 5]) for c in range(channels)],
                      ms=i & 1) for i in range(8)]
    return g.make_stream(blocks, channels=channels, bit_depth=24, stereo_mode=2 if channels == 2 else 0).lac


ESCAPE_N, ESCAPE_K = 300, 9


def escape_base(bit_depth, ptype=0, order=0):
    """One mono block, zero-run mode, every sample a 32-bit escape: token i starts at bit 31 + 34 i."""
    rng = _rng("escape%d%d" % (bit_depth, order))
    amp = 2000 if order == 0 else 20
    vals = [rng.randint(-amp, amp) for _ in range(ESCAPE_N)]
    cb = g.ChannelBlock(ESCAPE_N, ptype, order, [], 0, [g.Part(g.MODE_ZERO_RUN, ESCAPE_K, tokens=[("e", v) for v in vals])])
    return g.mono(cb, bit_depth=bit_depth).lac


def bases(block_end=None):
    out = {}
    for sub in ("small", "decode_wav"):
        for path in sorted(glob.glob(os.path.join(GOLDEN, sub, "*.lac"))):
            with open(path, "rb") as f:
                out[sub + "/" + os.path.basename(path)[:-4]] = f.read()
    for name in GRAMMAR_BASES:
        s = g.build(name)
        assert s.status == 0, name
        out[name] = s.lac
    out["equal_blocks_mono"] = equal_blocks("mono", 1)
    out["equal_blocks_stereo"] = equal_blocks("stereo", 2)
    out["escape_24"] = escape_base(24)
    out["escape_16_fixed1"] = escape_base(16, 0, 1)
    for name in V2_BASES:
        out["v2:" + name] = lacstreams.to_v2(out[name])
    return out


def _set_bits(buf, bitpos, nbits, value):
    for i in range(nbits):
        bit = (value >> (nbits - 1 - i)) & 1
        byte, sh = (bitpos + i) >> 3, 7 - ((bitpos + i) & 7)
        buf[byte] = (buf[byte] & ~(1 << sh)) | (bit << sh)


def _fill(rng, kind, n):
    return bytes([kind] * n) if kind is not None else bytes(rng.randrange(256) for _ in range(n))


def mutants_of(name, lac, block_end):
    """Yields (family, parameters, bytes) for one base."""
    version, ent, head = table(lac)
    nb, frames, size = len(ent), sum(n for n, _ in ent), len(lac)
    rng = _rng(name)
    small = frames <= SMALL_FRAMES
    exhaustive = small or nb <= FEW_BLOCKS
    weight = 1.0 if frames <= 1200 else (0.6 if small else 0.12)   # fewer random mutants of the long bases
    ends = []   # the last byte of every block (version 3) / of the stream
    off = head
    for _, s in ent:
        if s is not None:
            off += s
            ends.append(off - 1)
    if version == 2:
        ends = [size - 1]

    if version == 3 and exhaustive:  # ---- hdrflip
        seen = set()
        off = head
        for regions, (_, s) in zip(header_regions(lac, block_end), ent):
            spans = regions + [(off, min(off + 8, off + s)), (max(off, off + s - 8), off + s)]
            for a, b in spans:
                for pos in range(a, b):
                    if pos in seen:
                        continue
                    seen.add(pos)
                    for bit in range(8):
                        m = bytearray(lac)
                        m[pos] ^= 1 << bit
                        yield "hdrflip", "%d.%d" % (pos, bit), bytes(m)
            off += s

    for i in range(int(260 * weight)):  # ---- flip
        m = bytearray(lac)
        for _ in range(rng.randint(1, 4)):
            m[rng.randrange(head, size)] ^= 1 << rng.randrange(8)
        yield "flip", str(i), bytes(m)

    kinds = (0xFF, 0x00, 0xAA, None)
    for i in range(int(170 * weight)):  # ---- run
        n = rng.randint(1, 64)
        at = rng.randrange(head, size)
        m = bytearray(lac)
        fill = _fill(rng, kinds[i % 4], n)
        m[at:at + n] = fill[:size - at]
        yield "run", "r%d" % i, bytes(m)
    for e in sorted(set(ends[:3] + ends[-2:])):
        for kind in kinds:
            for n in (1, 7, rng.randint(2, 64), 64):
                a = max(head, e + 1 - n)
                m = bytearray(lac)
                m[a:e + 1] = _fill(rng, kind, e + 1 - a)
                yield "run", "end%d.%s.%d" % (e, kind, n), bytes(m)

    if version == 3 and nb > 1:  # ---- run: 64 bytes of 0xFF across a block seam, the block before it a multiple of 4 bytes long
        _, pays = _payloads(lac)  # (regression mutant `seam`: a unary run that ends exactly at the block's end must stop there)
        for b in (range(nb - 1) if nb <= 6 else sorted(rng.sample(range(nb - 1), 6))):
            d = len(pays[b]) % 4
            if len(pays[b]) - d < 40 or len(pays[b + 1]) < 40:
                continue
            p2 = list(pays)
            p2[b] = pays[b][:len(pays[b]) - d - 32] + b"\xff" * 32
            p2[b + 1] = b"\xff" * 32 + pays[b][len(pays[b]) - d:] + pays[b + 1][32:]
            yield "run", "seam%d" % b, _rebuild(lac, ent, p2)

    if version == 3 and nb > 1:  # ---- table, transplant
        _, pays = _payloads(lac)
        for b in range(nb - 1):
            for d in sorted({1, rng.randint(2, 40), 40}):
                for sign in (1, -1):
                    sa, sb = ent[b][1] + sign * d, ent[b + 1][1] - sign * d
                    if sa < 1 or sb < 1:
                        continue
                    e2 = list(ent)
                    e2[b], e2[b + 1] = (ent[b][0], sa), (ent[b + 1][0], sb)
                    yield "table", "%d%+d" % (b, sign * d), lacstreams._build(lac[:10], e2, lac[head:])
        combos = [(i, j) for i in range(nb) for j in range(nb) if i != j]
        if len(combos) > 60:
            combos = rng.sample(combos, 60)
        for i, j in combos:
            p2 = list(pays)
            p2[j] = pays[i]
            yield "transplant", "dup%d>%d" % (i, j), _rebuild(lac, ent, p2)
            if i < j and ent[i][0] != ent[j][0]:
                p2 = list(pays)
                p2[i], p2[j] = pays[j], pays[i]
                yield "transplant", "swap%d.%d" % (i, j), _rebuild(lac, ent, p2)

    if version == 3:  # ---- trunc
        _, pays = _payloads(lac)
        for b in (range(nb) if nb <= 4 else sorted(rng.sample(range(nb), 4))):
            for d in sorted({1, 2, rng.randint(3, 30), 30}):
                if len(pays[b]) > d:
                    p2 = list(pays)
                    p2[b] = pays[b][:-d]
                    yield "trunc", "cut%d.%d" % (b, d), _rebuild(lac, ent, p2)
                for kind in (0x00, 0xFF):
                    p2 = list(pays)
                    p2[b] = pays[b] + bytes([kind] * d)
                    yield "trunc", "ext%d.%d.%d" % (b, kind, d), _rebuild(lac, ent, p2)
            # regression mutant `lpc_header_at_block_end`: the block ends right behind an LPC header that announces 32
            # coefficients (64 bytes): the list must be refused before it is read
            flag = pays[b][:1] if (lac[3] == 2 and lac[4] == 2) else b""
            for keep in (0, 1, 5):
                p2 = list(pays)
                p2[b] = flag + bytes([2, 32]) + pays[b][len(flag) + 2:len(flag) + 2 + keep]
                yield "trunc", "lpc_header_at_block_end%d.%d" % (b, keep), _rebuild(lac, ent, p2)
    else:
        for d in (1, 2, 17, 30):
            yield "trunc", "cut.%d" % d, lac[:-d]
            yield "trunc", "ext0.%d" % d, lac + bytes(d)
            yield "trunc", "extff.%d" % d, lac + b"\xff" * d

    if name.startswith("escape_"):  # ---- escape: the 32 value bits of a token
        order = lac[head + 1]
        first = 8 * head + 24 + 7
        limit = (1 << (lac[8] - 1))
        extremes = [0, 1, 2 * limit - 2, 2 * limit - 1, 2 * limit, 2 * limit + 1, (1 << 30) - 1, 1 << 30, (1 << 30) + 1,
                    0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]
        for tok in (0, 1, 2, 3, 7, 100, 255, 256, 257, ESCAPE_N - 2, ESCAPE_N - 1):
            for v in extremes:
                m = bytearray(lac)
                _set_bits(m, first + 34 * tok + 2, 32, v)
                yield "escape", "tok%d.%x.o%d" % (tok, v, order), bytes(m)
    if version == 3 and exhaustive and block_end is not None:  # ---- escape: a partition's k
        off = head
        for b, (regions, (n, s)) in enumerate(zip(header_regions(lac, block_end), ent)):
            for c, (a, e) in enumerate(regions[-lac[3]:]):
                cb = lac[a:e]
                bits = 16 + (16 * cb[1] if cb[0] == 2 else 0)
                p = cb[bits // 8] & 0x0F
                parts = (1 << p) if (p and (n >> p)) else 1
                for part in sorted({0, 1, parts // 2, parts - 1} & set(range(parts))):
                    for k in (0, 1, 30, 31):
                        m = bytearray(lac)
                        _set_bits(m, 8 * a + bits + 8 + 7 * part + 2, 5, k)
                        yield "escape", "k%d.%d.%d.%d" % (b, c, part, k), bytes(m)
            off += s


_cache = {}


def corpus(block_end):
    """The whole corpus (cached): mutants that equal their base are left out."""
    if "c" not in _cache:
        out = []
        for name, lac in bases(block_end).items():
            seen = {lac}
            for family, params, m in mutants_of(name, lac, block_end):
                if m in seen:
                    continue
                seen.add(m)
                out.append(Mutant("%s|%s|%s" % (name, family, params), name, family, m))
        _cache["c"] = out
        _cache["bases"] = bases(block_end)
    return _cache["c"]


def base_of(mutant, block_end=None):
    corpus(block_end)
    return _cache["bases"][mutant.base]


def unchanged_blocks(base: bytes, lac: bytes):
    """Indices of the blocks of a version-3 mutant that have their base's table entry, place and bytes."""
    _, eb, hb = table(base)
    _, em, hm = table(lac)
    out, ob, om = [], hb, hm
    for b in range(min(len(eb), len(em))):
        if eb[b] == em[b] and ob - hb == om - hm and base[ob:ob + eb[b][1]] == lac[om:om + em[b][1]]:
            out.append(b)
        ob += eb[b][1]
        om += em[b][1]
    return out
