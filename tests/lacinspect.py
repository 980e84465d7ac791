"""The stream inspection restated in plain Python: the expectation for the rows of lacx_decoder_inspect_batch_device.

A parse-only walk of a .lac stream written from the format (the reference's docs/format.md) with lacgrammar's pieces
(Adapt, adapt_k, stateless_k, partition_sizes): which predictor, order and partition order every channel block has, the
mode of every partition, where the bits go (header, tags, unary, remainders, escapes, padding) and where the samples go
(Rice codes, zero runs, escapes, bin tags).  No sample is reconstructed, so the verdict of a block is one of the parse
codes 0 1 2 3 4 6 8 9 10 and never 5 or 7.

  inspect_stream(lac)      -> [row, ...] (one dict per block, the fields of lacx_block_info; ch: two dicts with the fields
                              of lacx_channel_info plus "partitions": [(mode_k, part_bits), ...]), or None where the
                              container's head cannot be read
  from_ctypes(row)         -> the same dict from a lacx.BlockInfo (its partitions where the row carries them)
  diff(have, want)         -> the differing fields of two lists of rows, as text
  report(rows, ...)        -> the totals as lacx_inspect_combine makes them, a dict with the fields of lacx_stream_report
  check_identities(row, stereo_flag)  asserts the identities the issue states on a block that parses
"""
from __future__ import annotations

import struct

from lacgrammar import Adapt, adapt_k, stateless_k

CH_SCALARS = ("predictor_type", "order", "partition_order", "k_min", "k_max", "bits", "header_bits", "tag_bits", "unary_bits",
              "remainder_bits", "escape_bits", "pad_bits", "rice_samples", "run_tokens", "run_samples", "escape_samples",
              "unary_max", "max_u", "sum_u")
CH_ARRAYS = ("coef", "bin_samples", "mode_parts", "mode_samples")
BIT_CLASSES = ("header_bits", "tag_bits", "unary_bits", "remainder_bits", "escape_bits", "pad_bits")
MISSING, NOT_REACHED = 10, 8
# what the walks of this process have met, for the tests that assert a corpus is not hollow: "stateful_run",
# "stateless_run", "run_ends_partition", ("mode", m, "block" | "partition"), "long_unary" (more than 64 bits)
SEEN = set()


def zero_channel():
    c = {k: 0 for k in CH_SCALARS}
    c.update(coef=[0] * 32, bin_samples=[0] * 3, mode_parts=[0] * 4, mode_samples=[0] * 4, partitions=[])
    return c


def lost_row(frames, nbytes, code):
    return dict(frames=frames, bytes=nbytes, code=code, ms=0, channels=0, ch=[zero_channel(), zero_channel()])


class Fault(Exception):
    def __init__(self, code):
        self.code = code


class _Reader:
    """MSB-first over `data`, positions in bits; what lies behind the end reads as zeros, and the caller checks pos
    against nbits where the decoder does (once per token: any token that reaches beyond the end is a fault whatever the
    bits were)."""

    def __init__(self, data):
        self.data = bytes(data) + b"\0" * 16
        self.nbits = 8 * len(data)
        self.pos = 0

    def peek(self, n):
        if n == 0:
            return 0
        b0, off = self.pos >> 3, self.pos & 7
        if b0 >= len(self.data) - 8:
            return 0
        return (int.from_bytes(self.data[b0:b0 + 8], "big") >> (64 - off - n)) & ((1 << n) - 1)

    def get(self, n):
        v = self.peek(n)
        self.pos += n
        return v

    def over(self):
        return self.pos > self.nbits

    def unary(self, max_q):
        """The quotient, or None where the ones run to the end of the block or beyond max_q."""
        q = 0
        while True:
            if self.pos >= self.nbits:
                return None
            v = self.peek(32)
            if v == 0xFFFFFFFF:
                q += 32
                self.pos += 32
                if q > max_q + 64:
                    return None
                continue
            ones = 32 - (v ^ 0xFFFFFFFF).bit_length()
            q += ones
            self.pos += ones + 1
            return q if q <= max_q else None


def _channel_block(r, n):
    """One channel block from r.pos -> its dict; Fault(code) where it does not parse."""
    c = zero_channel()
    start = r.pos
    ptype, order = r.get(8), r.get(8)
    if r.over() or ptype > 2:
        raise Fault(2)
    if ptype == 2:
        if order <= 0 or order > 32 or order >= n:
            raise Fault(2)
    elif ptype == 1:
        if order != 2:
            raise Fault(2)
    elif order > 4:
        raise Fault(2)
    if ptype == 2:
        if r.pos + 16 * order > r.nbits:
            raise Fault(2)
        for i in range(order):
            v = r.get(16)
            c["coef"][i] = v - 65536 if v >= 32768 else v
    control = r.get(8)
    if r.over() or control & 0x10:
        raise Fault(2)
    pflag, p, cmode = bool(control & 0x80), control & 0x0F, (control >> 5) & 3
    if (pflag and p == 0) or (not pflag and p != 0) or p > 8:
        raise Fault(2)
    if p > 0 and (n >> p) < 32:
        raise Fault(2)
    parts = 1 if (p == 0 or (n >> p) == 0) else 1 << p
    base = n if parts == 1 else n >> p
    if r.pos + 7 * parts > r.nbits:
        raise Fault(2)
    table = [(r.get(2), r.get(5)) for _ in range(parts)]
    stateless = p > 0
    c.update(predictor_type=ptype, order=order, partition_order=p, header_bits=r.pos - start, k_min=255, k_max=0)
    sizes = [base] * (parts - 1) + [n - base * (parts - 1)]
    for part, size in enumerate(sizes):
        mode, k = table[part]
        if part == 0 and mode != cmode:
            raise Fault(2)
        pos0 = r.pos
        c["mode_parts"][mode] += 1
        c["mode_samples"][mode] += size
        total = count = 0
        st = None if stateless else Adapt()

        def adapt(u):
            nonlocal total, count, k
            total += u
            count += 1
            k = stateless_k(total, count) if stateless else adapt_k(total, count, st)

        def rice(kk):
            q = r.unary(0xFFFFFFFF >> kk)
            if q is None:
                raise Fault(3)
            rem = r.get(kk)
            c["unary_bits"] += q + 1
            c["remainder_bits"] += kk
            c["unary_max"] = max(c["unary_max"], q)
            if q + 1 > 64:
                SEEN.add("long_unary")
            return (q << kk) | rem

        i = 0
        while i < size:
            tag = None
            if mode in (1, 2):
                tag = r.get(2)
                c["tag_bits"] += 2
            if mode == 1 and tag == 3:
                raise Fault(3)
            if mode == 1 and tag == 1:  # a run of zeros
                run = rice(2) + 4
                if run > size - i or r.over():
                    raise Fault(3)
                c["run_tokens"] += 1
                c["run_samples"] += run
                SEEN.add("stateless_run" if stateless else "stateful_run")
                if i + run == size:
                    SEEN.add("run_ends_partition")
                if stateless:
                    count += run
                    k = stateless_k(total, count)
                else:
                    for _ in range(run):
                        adapt(0)
                i += run
                continue
            if mode == 1 and tag == 2:
                u = r.get(32)
                c["escape_bits"] += 32
                c["escape_samples"] += 1
            elif mode == 2 and tag < 3:
                if tag == 0:
                    u = 0
                else:
                    sign = r.get(1)
                    c["remainder_bits"] += 1
                    u = 2 * tag - 1 if sign else 2 * tag
                c["bin_samples"][tag] += 1
            else:
                kk = k
                u = rice(kk)
                c["rice_samples"] += 1
                c["k_min"], c["k_max"] = min(c["k_min"], kk), max(c["k_max"], kk)
            if r.over():
                raise Fault(3)
            if u >> 30:
                raise Fault(9)
            c["max_u"] = max(c["max_u"], u)
            c["sum_u"] += u
            if mode != 3:
                adapt(u)
            i += 1
        c["partitions"].append(((mode << 5) | table[part][1], r.pos - pos0))
        SEEN.add(("mode", mode, "partition" if stateless else "block"))
    body_end = r.pos
    while r.pos & 7:
        if r.get(1) or r.over():
            raise Fault(4)
    c["pad_bits"] = r.pos - body_end
    c["bits"] = r.pos - start
    return c


def _block(r, n, channels, stereo_mode):
    """(ms, [channel dicts]) from r.pos; Fault."""
    ms = 1 if stereo_mode == 1 else 0
    if n == 0 or n > 16384:
        raise Fault(1)
    if channels == 2 and stereo_mode == 2:
        ms = r.get(8)
        if r.over() or ms > 1:
            raise Fault(1)
    return ms, [_channel_block(r, n) for _ in range(channels)]


def head(lac):
    """(version, channels, stereo_mode, sample_rate, bit_depth, [(frames, bytes or None), ...]) or None."""
    if len(lac) < 14 or lac[0] != 0x4C or lac[1] != 0x41 or lac[2] not in (2, 3):
        return None
    version, channels, sm, depth = lac[2], lac[3], lac[4], lac[8]
    rate = (lac[5] << 8) | lac[6] | (lac[7] << 16)
    nb = struct.unpack(">I", lac[10:14])[0]
    row = 4 if version == 2 else 8
    if nb == 0 or len(lac) < 14 + row * nb:
        return None
    table = []
    for b in range(nb):
        at = 14 + row * b
        table.append((struct.unpack(">I", lac[at:at + 4])[0], None if version == 2 else struct.unpack(">I", lac[at + 4:at + 8])[0]))
    return version, channels, sm, rate, depth, table


def inspect_stream(lac):
    h = head(lac)
    if h is None:
        return None
    version, channels, sm, _, _, table = h
    at = 14 + (4 if version == 2 else 8) * len(table)
    rows = []
    if version == 2:
        r = _Reader(lac[at:])
        failed = False
        for b, (n, _) in enumerate(table):
            if failed:
                rows.append(lost_row(n, 0, NOT_REACHED))
                continue
            pos0 = r.pos
            try:
                ms, chs = _block(r, n, channels, sm)
                if b + 1 == len(table) and r.pos != r.nbits:
                    raise Fault(6)
                rows.append(dict(frames=n, bytes=(r.pos - pos0) >> 3, code=0, ms=ms, channels=channels,
                                 ch=chs + [zero_channel()] * (2 - channels)))
            except Fault as f:
                rows.append(lost_row(n, 0, f.code))
                failed = True
        return rows
    for n, nbytes in table:
        if at + nbytes > len(lac):  # the file does not hold the block (and none behind it: the sizes are positive)
            rows.append(lost_row(n, nbytes, MISSING))
            at = len(lac) + 1
            continue
        r = _Reader(lac[at:at + nbytes])
        at += nbytes
        try:
            ms, chs = _block(r, n, channels, sm)
            if r.pos != r.nbits:
                raise Fault(6)
            rows.append(dict(frames=n, bytes=nbytes, code=0, ms=ms, channels=channels, ch=chs + [zero_channel()] * (2 - channels)))
        except Fault as f:
            rows.append(lost_row(n, nbytes, f.code))
    return rows


def from_ctypes(row):
    d = dict(frames=row.frames, bytes=row.bytes, code=row.code, ms=row.ms, channels=row.channels, ch=[])
    for c in range(2):
        s = row.ch[c]
        ch = {k: int(getattr(s, k)) for k in CH_SCALARS}
        ch.update({k: [int(x) for x in getattr(s, k)] for k in CH_ARRAYS})
        parts = getattr(row, "partitions", None)
        ch["partitions"] = None if parts is None else list(parts[c]) if c < len(parts) else []
        d["ch"].append(ch)
    return d


def diff(have, want):
    """The fields in which two lists of rows differ, as text for an assertion's message."""
    if len(have) != len(want):
        return "%d rows, expected %d" % (len(have), len(want))
    out = []
    for b, (h, w) in enumerate(zip(have, want)):
        out += ["block %d %s: %r, expected %r" % (b, k, h[k], w[k]) for k in h if k != "ch" and h[k] != w[k]]
        for c in range(2):
            out += ["block %d ch%d %s: %r, expected %r" % (b, c, k, h["ch"][c][k], w["ch"][c][k]) for k in h["ch"][c] if h["ch"][c][k] != w["ch"][c][k]]
    return "; ".join(out[:12])


def strip_partitions(rows):
    """The rows as a job without partition detail reports them."""
    return [dict(r, ch=[dict(c, partitions=None) for c in r["ch"]]) for r in rows]


def check_identities(row, stereo_flag):
    assert row["code"] == 0
    chs = row["ch"][:row["channels"]]
    for c in chs:
        assert sum(c[k] for k in BIT_CLASSES) == c["bits"], "the six bit classes sum to bits"
        assert c["rice_samples"] + c["run_samples"] + c["escape_samples"] + sum(c["bin_samples"]) == row["frames"] == sum(c["mode_samples"])
        assert sum(c["mode_parts"]) == (1 << c["partition_order"] if c["partition_order"] else 1)
        if c["partitions"] is not None:
            assert len(c["partitions"]) == sum(c["mode_parts"])
            assert c["header_bits"] + c["pad_bits"] + sum(b for _, b in c["partitions"]) == c["bits"]
    assert 8 * row["bytes"] == (8 if stereo_flag else 0) + sum(c["bits"] for c in chs)


def report(rows, info=None):
    """lacx_inspect_combine in Python.  info: (version, channels, stereo_mode, sample_rate, bit_depth, blocks) or None."""
    t = dict(frames=0, head_bytes=0, payload_bytes=0, sample_rate=0, channels=0, bit_depth=0, stereo_mode=0, version=0,
             blocks=len(rows), lost_blocks=0, ms_blocks=0, channel_blocks=0, fixed_blocks=[0] * 5, fir_blocks=0, lpc_blocks=[0] * 33,
             partition_order_blocks=[0] * 9, mode_parts=[0] * 4, mode_samples=[0] * 4, bits=0, flag_bits=0, header_bits=0, tag_bits=0,
             unary_bits=0, remainder_bits=0, escape_bits=0, pad_bits=0, rice_samples=0, run_tokens=0, run_samples=0, escape_samples=0,
             bin_samples=[0] * 3, sum_u=0, max_u=0, unary_max=0, k_min=255, k_max=0)
    if info is not None:
        version, channels, sm, rate, depth, blocks = info
        t.update(version=version, channels=channels, stereo_mode=sm, sample_rate=rate, bit_depth=depth,
                 head_bytes=14 + (4 if version == 2 else 8) * blocks)
    for r in rows:
        t["frames"] += r["frames"]
        if r["code"]:
            t["lost_blocks"] += 1
            continue
        t["payload_bytes"] += r["bytes"]
        t["ms_blocks"] += 1 if r["ms"] else 0
        chbits = 0
        for c in r["ch"][:r["channels"]]:
            t["channel_blocks"] += 1
            if c["predictor_type"] == 0:
                t["fixed_blocks"][c["order"]] += 1
            elif c["predictor_type"] == 1:
                t["fir_blocks"] += 1
            else:
                t["lpc_blocks"][c["order"]] += 1
            t["partition_order_blocks"][c["partition_order"]] += 1
            for m in range(4):
                t["mode_parts"][m] += c["mode_parts"][m]
                t["mode_samples"][m] += c["mode_samples"][m]
            for k in (*BIT_CLASSES, "rice_samples", "run_tokens", "run_samples", "escape_samples", "sum_u"):
                t[k] += c[k]
            for k in range(3):
                t["bin_samples"][k] += c["bin_samples"][k]
            chbits += c["bits"]
            t["max_u"], t["unary_max"] = max(t["max_u"], c["max_u"]), max(t["unary_max"], c["unary_max"])
            t["k_min"], t["k_max"] = min(t["k_min"], c["k_min"]), max(t["k_max"], c["k_max"])
        t["bits"] += chbits
        t["flag_bits"] += 8 * r["bytes"] - chbits
    return t


def report_from_ctypes(rep):
    t = {}
    for name, _ in rep._fields_:
        if name.startswith("reserved") or name in ("sum_u_lo", "sum_u_hi"):
            continue
        v = getattr(rep, name)
        t[name] = [int(x) for x in v] if hasattr(v, "__len__") else int(v)
    t["sum_u"] = (rep.sum_u_hi << 64) | rep.sum_u_lo
    return t
