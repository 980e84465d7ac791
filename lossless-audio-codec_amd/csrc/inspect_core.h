// inspect_core.h -- the per-lane code of the stream inspection (lacx.h): a parse-only walk of one channel
// block and of one block, over the bit reader and the Rice adaptation of decode_core.h as they are.  The adaptation
// depends on the residual magnitudes alone, never on reconstructed samples, so the walk takes the tokens, keeps a tally
// and synthesises nothing: no PCM, no predictor history, no coefficient column (the coefficients go to the row as they
// are read).  Shared by the gfx950 kernels of k_inspect.hip and the host twin (tests/native/sim_inspect.cpp).
//
// The grammar is decode_channel_block's, restated trip by trip -- one sample per trip, a zero run's zeros one per trip,
// the same order of checks -- so that the parameter in force at every token, the bounds argument of BitIn (every loop
// whose length the stream controls checks before it reads; overrun() once per trip) and the precedence of the fault
// codes are the decoder's.  What it cannot see: code 5 (sample overflow) and code 7 (outside the bit depth) need the
// samples, so the walk goes on where the decoder stops.  decode_channel_block itself is not touched and not shared:
// code that branches on its caller would change k_decode's instruction stream.
#pragma once
#include <cstdint>

#include "decode_core.h"
#include "lacx.h"

namespace lacx {

constexpr size_t kInspectBytesPerCol = 256 * 4;  // LDS per lane: the drift window of the stateful adaptation, nothing else

LACX_HDF DecMem inspect_mem(unsigned char* raw, uint32_t cols) {
    DecMem dm;
    dm.cols = cols;
    dm.ring_ = reinterpret_cast<uint32_t*>(raw);
    dm.hist_ = nullptr;
    dm.coef_ = nullptr;
    return dm;
}

// Where a lane leaves its findings: the block's row, and with LACX_INSPECT_PARTITIONS the two channel blocks' partition
// entries (mode_k: [2][256] bytes, part_bits: [2][256] words; null: not asked for).
struct InspectOut {
    lacx_block_info* row;
    uint8_t* mode_k;
    uint32_t* part_bits;
};

LACX_HDF void inspect_zero_words(void* p, uint32_t bytes) {
    uint32_t* w = static_cast<uint32_t*>(p);
    for (uint32_t i = 0; i < bytes / 4u; ++i) w[i] = 0u;
}

// One channel block (decode_channel_block without the synthesis).  c: the row to fill (all zero on entry; on a fault the
// caller zeroes it again), pmk / pbits: the channel block's partition entries or null.  0 = parses, else the code.
LACX_HDS uint32_t inspect_channel_block(BitIn& r, uint32_t n, lacx_channel_info* __restrict__ c, uint8_t* __restrict__ pmk,
                                        uint32_t* __restrict__ pbits, DecMem& dm, int lane) {
    const uint32_t start = r.pos;
    const uint32_t type = get_bits(r, 8);
    const int order = (int)get_bits(r, 8);
    if (overrun(r) || type > 2u) return 2;
    if (type == 2u) {
        if (order <= 0 || order > 32 || (uint32_t)order >= n) return 2;
    } else if (type == 1u) {
        if (order != 2) return 2;
    } else if (order > 4) {
        return 2;
    }
    if (type == 2u) {
        if (r.pos + 16u * (uint32_t)order > r.nbits) return 2;  // inside the block before a bit of it is fetched
        for (int i = 0; i < order; ++i) c->coef[i] = (int16_t)get_bits(r, 16);
        if (overrun(r)) return 2;
    }
    const uint32_t control = get_bits(r, 8);
    if (overrun(r) || (control & 0x10u)) return 2;
    const bool pflag = (control & 0x80u) != 0u;
    const uint32_t p = control & 0x0Fu, cmode = (control >> 5) & 3u;
    if ((pflag && p == 0u) || (!pflag && p != 0u) || p > (uint32_t)kMaxPartitionOrder) return 2;
    if (p > 0u && (n >> p) < (uint32_t)kMinPartition) return 2;
    const uint32_t parts = (p == 0u || (n >> p) == 0u) ? 1u : (1u << p);
    const uint32_t base = parts == 1u ? n : (n >> p);
    const uint32_t table_pos = r.pos;  // (mode:2, k:5) per partition, read when the partition starts
    if (r.pos + 7u * parts > r.nbits) return 2;
    reader_seek(r, r.pos + 7u * parts);
    const bool stateless = p > 0u;
    const uint32_t header_bits = r.pos - start;

    Adapt a;
    adapt_reset(a);
    uint32_t mode = 0, k = 0, seg_end = 0, part = 0, zeros_left = 0, st = 0;
    // the tally: bit classes, sample classes, extremes; the per-mode counters as four 16-bit fields of one word each
    // (at most 256 partitions and 16384 samples)
    uint32_t tag_bits = 0, unary_bits = 0, rem_bits = 0, esc_bits = 0;
    uint32_t rice = 0, run_tokens = 0, run_samples = 0, esc = 0, bin0 = 0, bin1 = 0, bin2 = 0;
    unsigned long long mode_parts = 0, mode_samples = 0, sum_u = 0;
    uint32_t k_min = 255, k_max = 0, unary_max = 0, max_u = 0;
    uint32_t part_pos = r.pos, part_entry = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (i == seg_end) {  // a partition starts (and the one before it ends)
            if (pmk && part) {
                pmk[part - 1u] = (uint8_t)part_entry;
                pbits[part - 1u] = r.pos - part_pos;
            }
            part_pos = r.pos;
            BitIn t = r;
            reader_seek(t, table_pos + 7u * part);
            mode = get_bits(t, 2);
            k = get_bits(t, 5);
            part_entry = (mode << 5) | k;
            if (part == 0u && mode != cmode) {
                st = 2;
                break;
            }
            seg_end += (part + 1u == parts) ? n - base * (parts - 1u) : base;
            ++part;
            adapt_reset(a);
            mode_parts += 1ull << (16u * mode);
        }
        // One token, whatever the grammar: [2-bit tag] [unary quotient] [remainder / sign / 32-bit escape]
        const bool in_run = zeros_left != 0u;
        zeros_left -= in_run ? 1u : 0u;
        const bool is_bin = mode == kModeBin, is_zr = mode == 1u;
        const bool tagged = !in_run && (is_bin || is_zr);
        refill(r);
        const uint32_t tag = tagged ? (uint32_t)(r.buf >> 62) : 0u;
        consume(r, tagged ? 2u : 0u);
        const bool run_token = tagged && is_zr && tag == 1u;
        const bool has_unary = !in_run && (!tagged || (is_bin ? tag == 3u : tag <= 1u));
        const uint32_t kk = run_token ? kZeroRunK : k;
        uint32_t bad = (tagged && is_zr && tag == 3u) ? 3u : 0u;
        uint32_t q = 0;
        {
            const unsigned long long inv = ~r.buf;  // the invalid low bits of buf are zero: they read as terminators
            const uint32_t ones = inv ? clz64(inv) : 64u;
            if (has_unary && ones >= r.have) {  // the run of ones goes on beyond the bits at hand (rare)
                if (!get_unary_slow(r, 0xFFFFFFFFu >> kk, q)) bad = 3u;
            } else {
                q = has_unary ? ones : 0u;
                consume(r, has_unary ? ones + 1u : 0u);
            }
            if (q > (0xFFFFFFFFu >> kk)) bad = 3u;
        }
        const bool escape = !in_run && !has_unary && is_zr && tag == 2u;
        const bool small_bin = tagged && is_bin && (tag == 1u || tag == 2u);  // +-1, +-2: tag and sign bit
        const uint32_t rem_n = in_run ? 0u : (has_unary ? kk : (small_bin ? 1u : (escape ? 32u : 0u)));
        if (r.have < rem_n) refill(r);
        const uint32_t rem = take(r, rem_n);
        const uint32_t value = has_unary ? ((q << kk) | rem) : rem;
        const uint32_t u = small_bin ? zigzag(rem ? -(int32_t)tag : (int32_t)tag) : ((run_token || in_run) ? 0u : value);
        bool adapt = mode != kModeStatic;  // a static partition keeps the k of its table entry
        if (in_run) adapt = !stateless;    // stateful streams adapt on every zero, stateless ones did it at the token
        if (run_token) {
            const unsigned long long run = (unsigned long long)value + kZeroRunMin;
            if (run > (unsigned long long)(seg_end - i)) bad = 3u;
            zeros_left = (uint32_t)run - 1u;
            run_samples += bad ? 0u : (uint32_t)run;
            if (stateless) {  // the count jumps by the run, the parameter is recomputed once
                a.count += (uint32_t)run;
                const uint32_t km = kmean(a.sum, a.count);
                k = km > 31u ? 31u : km;
                adapt = false;
            }
        }
        if (overrun(r)) bad = 3u;
        if (!bad && (u >> 30)) bad = 9u;
        if (bad) {
            st = bad;
            break;
        }
        // the tally of this trip
        const bool riced = has_unary && !run_token;
        tag_bits += tagged ? 2u : 0u;
        unary_bits += has_unary ? q + 1u : 0u;
        rem_bits += escape ? 0u : rem_n;
        esc_bits += escape ? 32u : 0u;
        rice += riced ? 1u : 0u;
        run_tokens += run_token ? 1u : 0u;
        esc += escape ? 1u : 0u;
        bin0 += (tagged && is_bin && tag == 0u) ? 1u : 0u;
        bin1 += (tagged && is_bin && tag == 1u) ? 1u : 0u;
        bin2 += (tagged && is_bin && tag == 2u) ? 1u : 0u;
        mode_samples += 1ull << (16u * mode);
        k_min = (riced && k < k_min) ? k : k_min;
        k_max = (riced && k > k_max) ? k : k_max;
        unary_max = q > unary_max ? q : unary_max;
        max_u = u > max_u ? u : max_u;
        sum_u += u;
        k = adapt_next(a, u, adapt, k, stateless, dm, lane);
    }
    if (st) return st;
    if (pmk && part) {  // the last partition ends with the samples
        pmk[part - 1u] = (uint8_t)part_entry;
        pbits[part - 1u] = r.pos - part_pos;
    }
    const uint32_t body_end = r.pos;
    while (r.pos & 7u) {  // zero padding to the byte
        if (get_bits(r, 1) || overrun(r)) return 4;
    }
    c->predictor_type = (uint8_t)type;
    c->order = (uint8_t)order;
    c->partition_order = (uint8_t)p;
    c->k_min = (uint8_t)k_min;
    c->k_max = (uint8_t)k_max;
    c->bits = r.pos - start;
    c->header_bits = header_bits;
    c->tag_bits = tag_bits;
    c->unary_bits = unary_bits;
    c->remainder_bits = rem_bits;
    c->escape_bits = esc_bits;
    c->pad_bits = r.pos - body_end;
    c->rice_samples = rice;
    c->run_tokens = run_tokens;
    c->run_samples = run_samples;
    c->escape_samples = esc;
    c->bin_samples[0] = bin0;
    c->bin_samples[1] = bin1;
    c->bin_samples[2] = bin2;
#pragma unroll
    for (uint32_t m = 0; m < 4u; ++m) {
        c->mode_parts[m] = (uint16_t)(mode_parts >> (16u * m));
        c->mode_samples[m] = (uint16_t)(mode_samples >> (16u * m));
    }
    c->unary_max = unary_max;
    c->max_u = max_u;
    c->sum_u = sum_u;
    return 0;
}

// One block from where the reader stands: the optional stereo flag and one or two channel blocks.  The row's channel
// records must be all zero on entry.  *ms: mid/side by flag or by stream mode.  0 = parses so far, else the code.
LACX_HDF uint32_t inspect_block(BitIn& r, uint32_t n, int channels, int stereo_mode, const InspectOut& o, uint32_t* ms, DecMem& dm,
                                int lane) {
    uint32_t st = 0;
    *ms = stereo_mode == 1 ? 1u : 0u;
    if (n == 0u || n > (uint32_t)kMaxBlock) st = 1;
    if (!st && channels == 2 && stereo_mode == 2) {  // per-block flag byte
        const uint32_t flag = get_bits(r, 8);
        if (overrun(r) || flag > 1u) st = 1;
        *ms = flag;
    }
    if (!st) st = inspect_channel_block(r, n, &o.row->ch[0], o.mode_k, o.part_bits, dm, lane);
    if (!st && channels == 2)
        st = inspect_channel_block(r, n, &o.row->ch[1], o.mode_k ? o.mode_k + kInspectPartSlots : nullptr,
                                   o.part_bits ? o.part_bits + kInspectPartSlots : nullptr, dm, lane);
    return st;
}

// The row's head once the verdict is known; a block that does not parse keeps frames, bytes and code only (its partition
// entries too are zeroed: nothing of a faulted block is reported).
LACX_HDF void inspect_finish(const InspectOut& o, uint32_t frames, uint32_t bytes, uint32_t code, uint32_t ms, int channels) {
    lacx_block_info* row = o.row;
    if (code) {
        inspect_zero_words(row, (uint32_t)sizeof(lacx_block_info));
        if (o.mode_k) {
            inspect_zero_words(o.mode_k, 2u * kInspectPartSlots);
            inspect_zero_words(o.part_bits, 2u * kInspectPartSlots * 4u);
        }
    }
    row->frames = frames;
    row->bytes = bytes;
    row->code = code;
    row->ms = code ? 0u : (uint8_t)ms;
    row->channels = code ? 0u : (uint8_t)channels;
}

LACX_HDF InspectOut inspect_out(uint32_t blk, lacx_block_info* rows, uint8_t* mode_k, uint32_t* part_bits) {
    InspectOut o;
    o.row = rows + blk;
    o.mode_k = mode_k ? mode_k + (size_t)blk * 2u * kInspectPartSlots : nullptr;
    o.part_bits = part_bits ? part_bits + (size_t)blk * 2u * kInspectPartSlots : nullptr;
    return o;
}

// One block of a version-3 stream by one lane (k_inspect): blk indexes the global tables and the rows.
LACX_HDF void inspect_block_lane(uint32_t blk, int channels, int stereo_mode, const uint8_t* __restrict__ payload,
                                 const unsigned long long* __restrict__ byte_off, const unsigned long long* __restrict__ frame_off,
                                 lacx_block_info* __restrict__ rows, uint8_t* __restrict__ mode_k, uint32_t* __restrict__ part_bits,
                                 DecMem& dm, int lane, DecWave& wave) {
    const uint32_t n = (uint32_t)(frame_off[blk + 1] - frame_off[blk]);
    const uint32_t bytes = (uint32_t)(byte_off[blk + 1] - byte_off[blk]);
    const InspectOut o = inspect_out(blk, rows, mode_k, part_bits);
    inspect_zero_words(o.row, (uint32_t)sizeof(lacx_block_info));
    BitIn r;
    reader_init(r, payload + byte_off[blk], 8u * bytes, wave);
    uint32_t ms = 0;
    uint32_t st = inspect_block(r, n, channels, stereo_mode, o, &ms, dm, lane);
    if (!st && r.pos != r.nbits) st = 6;  // trailing bytes in the block
    inspect_finish(o, n, bytes, st, ms, channels);
}

// Blocks [0, num_blocks) of one version-2 stream by one lane, in order (k_inspect_serial): a block's bytes are what the
// walk found; the blocks behind the first that fails get 8 (not reached).  rows / mode_k / part_bits: the stream's own.
LACX_HDF void inspect_serial_lane(uint32_t num_blocks, int channels, int stereo_mode, const uint8_t* __restrict__ payload,
                                  uint32_t payload_bits, const unsigned long long* __restrict__ frame_off,
                                  lacx_block_info* __restrict__ rows, uint8_t* __restrict__ mode_k, uint32_t* __restrict__ part_bits,
                                  DecMem& dm, int lane, DecWave& wave) {
    BitIn r;
    reader_init(r, payload, payload_bits, wave);
    uint32_t failed = 0;
    for (uint32_t blk = 0; blk < num_blocks; ++blk) {
        const uint32_t n = (uint32_t)(frame_off[blk + 1] - frame_off[blk]);
        const InspectOut o = inspect_out(blk, rows, mode_k, part_bits);
        inspect_zero_words(o.row, (uint32_t)sizeof(lacx_block_info));
        if (failed) {
            inspect_finish(o, n, 0u, 8u, 0u, channels);  // not reached
            continue;
        }
        const uint32_t pos0 = r.pos;
        uint32_t ms = 0;
        uint32_t st = inspect_block(r, n, channels, stereo_mode, o, &ms, dm, lane);
        if (!st && blk + 1u == num_blocks && r.pos != r.nbits) st = 6;  // trailing frame payload
        inspect_finish(o, n, st ? 0u : (r.pos - pos0) >> 3, st, ms, channels);
        failed = st;
    }
}

}  // namespace lacx
