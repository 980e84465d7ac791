// api_decode.cpp -- the decode entry points of the C ABI: container parsing and the device decoder's host side.
#include "encoder_impl.h"

extern "C" {

// ---- decode -------------------------------------------------------------------------------------
namespace {
thread_local std::string g_decode_err;
int decode_fail(int code, const std::string& msg) {
    g_decode_err = msg;
    return code;
}
uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
}  // namespace

const char* lacx_decode_last_error(void) { return g_decode_err.c_str(); }

// Container header + block table: the structural rules of the reference's reader (src/codec/frame/frame_header.hpp:48-74,
// lac/decoder.cpp:84-145) -- sync, version 3, channels, stereo mode (0 for mono), one of the four sample rates, depth,
// reserved byte; at least one block; every block 1..16384 frames, non-final ones at least 256; non-zero compressed
// sizes that add up to the file; at most 6 912 000 000 samples and a WAV that RIFF can hold.  NOT taken over: its cap on
// the decoded PCM (1 GiB) and the block count that follows from it, which would refuse the 2 h stream of BASELINE
// configs[3].  The legacy version-2 container (no compressed sizes, hence no parallelism) is read too: one lane walks it.
int lacx_stream_parse(const uint8_t* lac, uint64_t size, lacx_stream_info* out) {
    if (!lac || !out) return decode_fail(LACX_E_INVALID, "null argument");
    if (size == 0) return decode_fail(LACX_E_INVALID, "[decode-error] empty input");
    if (size < 10 || lac[0] != 0x4C || lac[1] != 0x41 || (lac[2] != 3 && lac[2] != 2))
        return decode_fail(LACX_E_INVALID, "[decode-error] invalid frame header");
    const int version = lac[2], ch = lac[3], sm = lac[4], bd = lac[8];
    const uint32_t sr = ((uint32_t)lac[5] << 8) | lac[6] | ((uint32_t)lac[7] << 16);
    const bool rate_ok = sr == 44100 || sr == 48000 || sr == 96000 || sr == 192000;
    if ((ch != 1 && ch != 2) || sm > 2 || (ch == 1 && sm != 0) || !rate_ok || (bd != 16 && bd != 24) || lac[9] != 0)
        return decode_fail(LACX_E_INVALID, "[decode-error] invalid frame header");
    if (size < 14) return decode_fail(LACX_E_INVALID, "[decode-error] invalid block count");
    const uint32_t nb = be32(lac + 10);
    if (nb == 0) return decode_fail(LACX_E_INVALID, "[decode-error] invalid block count");
    const uint64_t entry = version >= 3 ? 8u : 4u;  // version 2 has no compressed sizes (ref lac/decoder.cpp:100-104)
    if (size < 14 + entry * nb) return decode_fail(LACX_E_INVALID, "[decode-error] truncated block size table");
    uint64_t frames = 0, pay = 0;
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t n = be32(lac + 14 + entry * b);
        if (n == 0 || n > (uint32_t)kMaxBlock || (b + 1 < nb && n < 256u)) return decode_fail(LACX_E_INVALID, "[decode-error] invalid block size");
        frames += n;
        if (frames > 6912000000ull) return decode_fail(LACX_E_INVALID, "[decode-error] total samples exceed maximum");
        if (version >= 3) {
            const uint32_t by = be32(lac + 18 + 8ull * b);
            // The device reader's bit positions are 32-bit and relative to the block: a block must stay below 2^29 bytes.
            // (The reference takes any non-zero size that fits the file; a block this long -- a Rice token at k = 0 may
            // carry a unary part of up to 2^30 bits -- is a documented deviation, see lacx.h.)
            if (by == 0 || by >= (1u << 29)) return decode_fail(LACX_E_INVALID, "[decode-error] invalid compressed block size");
            pay += by;
            if (pay > size) return decode_fail(LACX_E_INVALID, "[decode-error] compressed block sizes exceed frame payload");
        }
    }
    const uint64_t wav_bytes = frames * (uint64_t)ch * (uint64_t)(bd / 8);
    if (36u + wav_bytes + (wav_bytes & 1u) > 0xFFFFFFFFull) return decode_fail(LACX_E_INVALID, "[decode-error] decoded WAV data exceeds RIFF limit");
    if (version >= 3 && 14 + 8ull * nb + pay != size) return decode_fail(LACX_E_INVALID, "[decode-error] block payloads do not fill the file");
    if (version == 2 && size - (14 + 4ull * nb) >= (1ull << 29)) return decode_fail(LACX_E_INVALID, "[decode-error] version-2 payload too large for the serial reader");
    out->sample_rate = sr;
    out->blocks = nb;
    out->frames = frames;
    out->channels = (uint8_t)ch;
    out->bit_depth = (uint8_t)bd;
    out->stereo_mode = (uint8_t)sm;
    out->version = (uint8_t)version;
    return LACX_OK;
}

// The decoder object: device buffers, a stream and two events that live from call to call (grow-only), so that a decode
// costs its copies and its kernel, not six allocations (ref LAC::Decoder is an object too, src/codec/lac/decoder.hpp:10-24).
struct lacx_decoder {
    int device = -1;  // -1: whatever device is current at the first call
    bool ready = false;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    uint8_t* d_pay = nullptr;
    uint64_t pay_cap = 0;
    uint8_t* h_pay = nullptr;  // pinned: the window form's payload ranges, gathered for one H2D copy
    uint64_t h_pay_cap = 0;
    int32_t *d_left = nullptr, *d_right = nullptr;
    uint64_t pcm_cap = 0;
    uint32_t* d_status = nullptr;
    uint8_t* d_ms = nullptr;
    uint32_t* h_status = nullptr;  // pinned
    uint32_t blocks_cap = 0;
    uint8_t* d_wav = nullptr;  // WAV image (lacx_decoder_decode_wav*): header + data + pad
    uint8_t* h_wav = nullptr;  // pinned, behind lacx_decoder_decode_wav_view
    uint64_t wav_cap = 0;      // bytes of each
    uint8_t* d_meta = nullptr;  // item descriptors, offsets and lane tables (one upload)
    uint8_t* h_meta = nullptr;  // pinned
    uint64_t meta_cap = 0;      // bytes of each
    std::vector<std::string> item_err;  // the last batch call's message per item ("" = decoded)
    std::string err;
};

namespace {
void decoder_release(lacx_decoder* d) {
    if (d->ready) (void)hipSetDevice(d->device);
    if (d->e0) (void)hipEventDestroy(d->e0);
    if (d->e1) (void)hipEventDestroy(d->e1);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    if (d->d_pay) (void)hipFree(d->d_pay);
    if (d->h_pay) (void)hipHostFree(d->h_pay);
    if (d->d_left) (void)hipFree(d->d_left);
    if (d->d_right) (void)hipFree(d->d_right);
    if (d->d_status) (void)hipFree(d->d_status);
    if (d->d_ms) (void)hipFree(d->d_ms);
    if (d->h_status) (void)hipHostFree(d->h_status);
    if (d->d_wav) (void)hipFree(d->d_wav);
    if (d->h_wav) (void)hipHostFree(d->h_wav);
    if (d->d_meta) (void)hipFree(d->d_meta);
    if (d->h_meta) (void)hipHostFree(d->h_meta);
    *d = lacx_decoder{};
}
// lacx_decode (no handle): one decoder per device for the life of the process (never freed: releasing device memory from
// a static or thread-local destructor would race the HIP runtime's own shutdown), calls on one device take turns
struct SharedDecoder {
    std::mutex mu;
    lacx_decoder dec;
};
constexpr int kMaxDecodeDevices = 64;
std::mutex g_shared_mu;
SharedDecoder* g_shared[kMaxDecodeDevices] = {};
}  // namespace

int lacx_decoder_create(int device, lacx_decoder** out) {
    if (!out) return LACX_E_INVALID;
    lacx_decoder* d = new lacx_decoder();
    d->device = device;
    *out = d;
    return LACX_OK;
}

void lacx_decoder_destroy(lacx_decoder* d) {
    if (!d) return;
    decoder_release(d);
    delete d;
}

namespace {
// The 44-byte canonical header of the decoded WAV (ref src/main.cpp:127-148, 248-262); returns the image's size.
uint64_t wav_header(const lacx_stream_info& info, uint8_t* h) {
    const uint32_t align = (uint32_t)info.channels * (info.bit_depth / 8u);
    const uint64_t data = info.frames * align, pad = data & 1u;
    auto u16 = [&](int at, uint32_t v) { h[at] = (uint8_t)v, h[at + 1] = (uint8_t)(v >> 8); };
    auto u32 = [&](int at, uint32_t v) { u16(at, v & 0xFFFFu), u16(at + 2, v >> 16); };
    std::memcpy(h, "RIFF", 4);
    u32(4, (uint32_t)(36u + data + pad));  // below 2^32: lacx_stream_parse's RIFF limit
    std::memcpy(h + 8, "WAVEfmt ", 8);
    u32(16, 16);
    u16(20, 1);
    u16(22, info.channels);
    u32(24, info.sample_rate);
    u32(28, info.sample_rate * align);
    u16(32, align);
    u16(34, info.bit_depth);
    std::memcpy(h + 36, "data", 4);
    u32(40, (uint32_t)data);
    return 44u + data + pad;
}

// The decoder's grow-only buffers.  Each returns the failing call's error and names it in *what.
hipError_t decoder_open(lacx_decoder* d, int* prev_device, const char** what) {  // *prev_device: to put back, or -1
    hipError_t e = hipSuccess;
    *prev_device = -1;
    if (!d->ready && d->device < 0 && (e = hipGetDevice(&d->device)) != hipSuccess) return *what = "hipGetDevice", e;
    int cur = -1;
    if ((e = hipGetDevice(&cur)) != hipSuccess) return *what = "hipGetDevice", e;
    if (cur != d->device) {
        if ((e = hipSetDevice(d->device)) != hipSuccess) return *what = "hipSetDevice", e;
        *prev_device = cur;
    }
    if (!d->ready) {
        if ((e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking)) != hipSuccess) return *what = "hipStreamCreate", e;
        if ((e = hipEventCreate(&d->e0)) != hipSuccess) return *what = "hipEventCreate", e;
        if ((e = hipEventCreate(&d->e1)) != hipSuccess) return *what = "hipEventCreate", e;
        d->ready = true;
    }
    return e;
}
hipError_t grow_payload(lacx_decoder* d, uint64_t pay, const char** what) {  // pay bytes + the reader's tail pad
    if (pay + kDecodeTailPad <= d->pay_cap) return hipSuccess;
    if (d->d_pay) (void)hipFree(d->d_pay);
    d->d_pay = nullptr;
    d->pay_cap = 0;
    const uint64_t cap = pay + pay / 8 + kDecodeTailPad;
    *what = "hipMalloc(payload)";
    const hipError_t e = hipMalloc((void**)&d->d_pay, cap);
    if (e == hipSuccess) d->pay_cap = cap;
    return e;
}
hipError_t grow_pay_stage(lacx_decoder* d, uint64_t pay, const char** what) {  // pinned twin of the payload buffer
    if (pay <= d->h_pay_cap) return hipSuccess;
    if (d->h_pay) (void)hipHostFree(d->h_pay);
    d->h_pay = nullptr;
    d->h_pay_cap = 0;
    const uint64_t cap = pay + pay / 8 + 4096;
    *what = "hipHostMalloc(payload stage)";
    const hipError_t e = hipHostMalloc((void**)&d->h_pay, cap, 0);
    if (e == hipSuccess) d->h_pay_cap = cap;
    return e;
}
// dst[off[j], off[j] + bytes[j]) = src[j][0, bytes[j]) for every j, the destination split into equal byte ranges over up
// to 8 threads (the calling thread takes the first): a window batch is many short ranges of different streams, which as
// one pageable copy each would cost 10-20 us apiece in the runtime.
void gather_ranges(uint8_t* dst, const std::vector<const uint8_t*>& src, const std::vector<uint64_t>& off,
                   const std::vector<uint64_t>& bytes, uint64_t total) {
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned nt = total < (8u << 20) ? 1u : std::max(1u, std::min(8u, hw));
    auto part = [&](unsigned t) {
        const uint64_t lo = total * t / nt, hi = total * (t + 1) / nt;
        for (size_t j = 0; j < src.size(); ++j) {
            const uint64_t a = std::max(lo, off[j]), b = std::min(hi, off[j] + bytes[j]);
            if (a < b) std::memcpy(dst + a, src[j] + (a - off[j]), b - a);
        }
    };
    std::vector<std::thread> pool;
    unsigned t = 1;
    try {
        for (; t < nt; ++t) pool.emplace_back(part, t);
    } catch (...) {  // no thread to be had: the calling thread copies what is left
        for (unsigned u = t; u < nt; ++u) part(u);
    }
    part(0);
    for (auto& th : pool) th.join();
}

hipError_t grow_blocks(lacx_decoder* d, uint32_t nb, const char** what) {
    if (nb <= d->blocks_cap) return hipSuccess;
    if (d->d_status) (void)hipFree(d->d_status);
    if (d->d_ms) (void)hipFree(d->d_ms);
    if (d->h_status) (void)hipHostFree(d->h_status);
    d->d_status = nullptr;
    d->d_ms = nullptr;
    d->h_status = nullptr;
    d->blocks_cap = 0;
    const uint32_t cap = nb + nb / 8 + 16;
    hipError_t e;
    if ((e = hipMalloc((void**)&d->d_status, (size_t)cap * sizeof(uint32_t))) != hipSuccess) return *what = "hipMalloc(status)", e;
    if ((e = hipMalloc((void**)&d->d_ms, cap)) != hipSuccess) return *what = "hipMalloc(flags)", e;
    if ((e = hipHostMalloc((void**)&d->h_status, (size_t)cap * sizeof(uint32_t), 0)) != hipSuccess) return *what = "hipHostMalloc(status)", e;
    d->blocks_cap = cap;
    return e;
}
hipError_t grow_wav(lacx_decoder* d, uint64_t bytes, const char** what) {  // device and pinned image buffers
    if (bytes <= d->wav_cap) return hipSuccess;
    if (d->d_wav) (void)hipFree(d->d_wav);
    if (d->h_wav) (void)hipHostFree(d->h_wav);
    d->d_wav = d->h_wav = nullptr;
    d->wav_cap = 0;
    const uint64_t cap = (bytes + 15u) & ~15ull;  // k_wav_pack writes whole dwords, and only inside the image
    hipError_t e;
    if ((e = hipMalloc((void**)&d->d_wav, cap)) != hipSuccess) return *what = "hipMalloc(wav)", e;
    if ((e = hipHostMalloc((void**)&d->h_wav, cap, 0)) != hipSuccess) return *what = "hipHostMalloc(wav)", e;
    d->wav_cap = cap;
    return e;
}
hipError_t grow_pcm(lacx_decoder* d, uint64_t frames, const char** what) {  // both channels, whatever the stream's count
    if (frames <= d->pcm_cap && d->d_right) return hipSuccess;
    if (d->d_left) (void)hipFree(d->d_left);
    if (d->d_right) (void)hipFree(d->d_right);
    d->d_left = d->d_right = nullptr;
    d->pcm_cap = 0;
    hipError_t e;
    if ((e = hipMalloc((void**)&d->d_left, frames * sizeof(int32_t))) != hipSuccess) return *what = "hipMalloc(left)", e;
    if ((e = hipMalloc((void**)&d->d_right, frames * sizeof(int32_t))) != hipSuccess) return *what = "hipMalloc(right)", e;
    d->pcm_cap = frames;
    return e;
}

const char* block_error(uint32_t st) {
    static const char* const kWhat[] = {"", "block header", "channel header", "residual", "padding", "sample overflow",
                                        "trailing bytes", "sample outside the bit depth", "not reached", "residual beyond 2^30"};
    return st < 10 ? kWhat[st] : "?";
}

// One item of a decode: the stream, and for the device and host forms the caller's output arrays.  The window form
// (decode_batch_run's `window` >= 0): frames [start, start + frames) of the stream, as that sample type.
struct BatchIn {
    const uint8_t* lac;
    uint64_t size;
    int32_t* left;
    int32_t* right;
    uint64_t frames;
    uint64_t start = 0;
    // verify form: the source PCM (device-resident), or -- lacx_decoder_verify_wav, a batch of one -- the WAV data chunk
    // in host memory, which the decoder uploads behind the payload and pcm.data0 then points at
    lacx_pcm pcm = {nullptr, nullptr, 0, 0};
    const uint8_t* host_src = nullptr;
    uint64_t host_src_bytes = 0;
};

// Where the decoded items go.  wav: the images into the decoder's pinned image buffer (out[i]: each item's, 16-byte
// aligned, one D2H copy for all).  device: the caller's device arrays, in place, on the caller's stream.  host: the
// decoder's own PCM buffers, then, once the statuses are checked, the caller's host arrays of the items that decoded.
// verify: the decoder's own PCM buffers, compared there with each item's source PCM (k_verify in place of the other post
// passes, on the caller's stream); what comes back is vres[i] and, for an item that differs, LACX_E_MISMATCH.
enum class DecodeTo { wav, device, host, verify };

// The decoder: n streams as one decode (a single stream is n = 1).  Every item is parsed on the host first; those that
// parse go to the device together: their payloads back to back in one buffer (the tail pad after the last), their block
// tables as global prefix sums, one lane per version-3 block (an item's blocks in consecutive lanes) and one lane per
// version-2 item, then one post pass over all of them.  Per item, code[i] and err[i] ("" = decoded): the message its
// decode gives.  Returns LACX_OK, or LACX_E_DEVICE for a failure of the whole call (every item that parsed then carries
// it).  The caller decides what the outcome becomes: the batch entry points keep it in d->item_err.
// window = LACX_SAMPLE_I32 / _F32 (device or host form): each item's window only.  A version-3 item then
// covers just the blocks that overlap its window -- only their bytes are uploaded, they decode whole into the decoder's
// PCM buffers (scratch) and are all checked, and k_window_out writes the window's frames out; a version-2 item (no
// compressed sizes) decodes in full and is then windowed.  The host form's windows go through the decoder's image
// buffer, copied to the caller once the statuses are checked.
int decode_batch_run(lacx_decoder* d, const BatchIn* in, uint32_t n, DecodeTo to, hipStream_t stream, lacx_span* out,
                     std::vector<int>& code, std::vector<std::string>& err, float* device_ms, int window = -1,
                     lacx_verify_result* vres = nullptr) {
    if (device_ms) *device_ms = 0.f;
    const bool wav = to == DecodeTo::wav, own_pcm = to != DecodeTo::device || window >= 0;  // own_pcm: into d->d_left / d_right
    const bool verify = to == DecodeTo::verify;
    if (vres) std::memset(vres, 0, sizeof(lacx_verify_result) * n);
    code.assign(n, LACX_OK);
    err.assign(n, std::string());
    std::vector<lacx_stream_info> info(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (out) out[i] = lacx_span{nullptr, 0};
        int c = lacx_stream_parse(in[i].lac, in[i].size, &info[i]);
        if (c == LACX_OK && window >= 0) {  // the window inside the stream (no wrap-around), then the output arrays
            const uint64_t total = info[i].frames;
            if (in[i].frames == 0) c = decode_fail(LACX_E_INVALID, "empty window");
            else if (in[i].start >= total || in[i].frames > total - in[i].start) c = decode_fail(LACX_E_INVALID, "window outside the stream");
            else if (!in[i].left || (info[i].channels == 2 && !in[i].right)) c = decode_fail(LACX_E_INVALID, "output arrays missing");
        } else if (c == LACX_OK && verify) {  // the source against the stream
            const lacx_pcm& p = in[i].pcm;
            const uintptr_t a0 = (uintptr_t)p.data0, a1 = (uintptr_t)p.data1;
            const bool planar = p.layout == LACX_PCM_PLANAR_I32;
            if (p.layout > LACX_PCM_INTERLEAVED_I24) c = decode_fail(LACX_E_INVALID, "unknown source layout");
            else if (p.channels != info[i].channels) c = decode_fail(LACX_E_INVALID, "source channel count does not match the stream");
            else if ((!p.data0 && !in[i].host_src) || (planar && p.channels == 2 && !p.data1)) c = decode_fail(LACX_E_INVALID, "source arrays missing");
            else if (in[i].frames != info[i].frames) c = decode_fail(LACX_E_INVALID, "source frame count does not match the stream");
            else if ((p.layout == LACX_PCM_INTERLEAVED_I16 && info[i].bit_depth != 16) ||
                     (p.layout == LACX_PCM_INTERLEAVED_I24 && info[i].bit_depth != 24))
                c = decode_fail(LACX_E_INVALID, "source layout does not match the stream's bit depth");
            else if ((p.layout != LACX_PCM_INTERLEAVED_I24 && (a0 & 3u)) || (planar && (a1 & 3u)))
                c = decode_fail(LACX_E_INVALID, "source arrays are not 4-byte aligned");
        } else if (c == LACX_OK && !wav) {  // lacx_decoder_decode's checks of the output arrays
            if (!in[i].left || (info[i].channels == 2 && !in[i].right)) c = decode_fail(LACX_E_INVALID, "output arrays missing");
            else if (in[i].frames != info[i].frames)
                c = decode_fail(LACX_E_INVALID, "output arrays do not match the stream's frame count");
        }
        if (c != LACX_OK) {
            code[i] = c;
            err[i] = g_decode_err;
        }
    }
    // the items that go to the device, and where each one lies in the batch's buffers
    std::vector<uint32_t> dev;
    std::vector<DecodeItem> it;
    std::vector<uint64_t> pcm_at, wav_at, image_size;
    uint64_t total_blocks = 0, total_frames = 0, total_pay = 0, total_units = 0, pcm_total = 0, image_total = 0;
    uint32_t v3_blocks = 0;
    // what an item decodes: its blocks from blk_first on, and their payload bytes from pay_src on (both 0 and the whole
    // stream but in the window form); win: the window form's outputs, win_at: the host form's place in d->d_wav
    std::vector<uint32_t> blk_first;
    std::vector<uint64_t> pay_src, pay_bytes, win_at;
    std::vector<WindowOut> win;
    for (uint32_t i = 0; i < n; ++i) {
        if (code[i] != LACX_OK) continue;
        const lacx_stream_info& f = info[i];
        const uint64_t head = 14 + (f.version == 2 ? 4ull : 8ull) * f.blocks;
        uint32_t b0 = 0, nb = f.blocks;
        uint64_t src = 0, bytes = in[i].size - head, frames = f.frames, fr0 = 0;
        if (window >= 0 && f.version != 2) {  // the blocks [b0, b0 + nb) that hold the window's first and last frames
            const uint64_t last = in[i].start + in[i].frames - 1;
            uint64_t fr = 0, by = 0;
            for (uint32_t b = 0;; ++b) {  // (the parse guarantees that the window's last frame lies in a block)
                const uint32_t nfr = be32(in[i].lac + 14 + 8ull * b), nby = be32(in[i].lac + 18 + 8ull * b);
                if (fr <= in[i].start && in[i].start < fr + nfr) b0 = b, src = by, fr0 = fr;
                if (last < fr + nfr) {
                    nb = b + 1 - b0;
                    bytes = by + nby - src;
                    frames = fr + nfr - fr0;
                    break;
                }
                fr += nfr;
                by += nby;
            }
        }
        if (window >= 0) {
            const uint64_t out_words = in[i].frames * f.channels;  // the host form's staging: left, then right
            win.push_back(WindowOut{in[i].left, f.channels == 2 ? in[i].right : nullptr, in[i].start - fr0, in[i].frames});
            win_at.push_back(image_total);
            image_total += 4 * out_words;
            total_units += (frames + 3u) / 4u;
        }
        if (verify) total_units += (frames + 3u) / 4u;
        blk_first.push_back(b0);
        pay_src.push_back(src);
        pay_bytes.push_back(bytes);
        DecodeItem x{};
        x.frame0 = total_frames;
        x.frames = frames;
        x.pay_off = total_pay;
        x.block0 = (uint32_t)total_blocks;
        x.blocks = nb;
        x.pay_bits = f.version == 2 ? (uint32_t)(8ull * (in[i].size - head)) : 0u;  // < 2^32: lacx_stream_parse
        x.channels = f.channels;
        x.stereo_mode = f.stereo_mode;
        x.bit_depth = f.bit_depth;
        x.version = f.version;
        if (own_pcm) {  // offsets for now, pointers once the buffers exist
            pcm_at.push_back(pcm_total);
            pcm_total += (frames + 3u) & ~3ull;  // every item's PCM from a multiple of 4 frames: 16-byte loads
        }
        if (wav) {
            uint8_t hdr[44];
            const uint64_t image = wav_header(f, hdr);
            wav_at.push_back(image_total);
            image_size.push_back(image);
            image_total += (image + 15u) & ~15ull;
            total_units += (f.frames + 3u) / 4u;
        }
        if (!own_pcm) {
            x.left = in[i].left;
            x.right = f.channels == 2 ? in[i].right : nullptr;
        }
        total_blocks += nb;
        total_frames += frames;
        total_pay += bytes;
        if (f.version != 2) v3_blocks += nb;
        dev.push_back(i);
        it.push_back(x);
    }
    const char* no_device = lacx_device_count() <= 0 ? "no usable HIP device" : nullptr;
    if (!no_device && total_blocks >= (1ull << 31)) no_device = "batch holds 2^31 blocks or more";
    int rc = LACX_OK;
    int prev_device = -1;
    const uint32_t m = (uint32_t)dev.size();
    if (no_device) {
        rc = decode_fail(LACX_E_DEVICE, no_device);
    } else if (m > 0) {
#define DEC_TRY(call, what)                                                                                  \
    do {                                                                                                     \
        const hipError_t _e = (call);                                                                        \
        if (_e != hipSuccess) {                                                                              \
            rc = decode_fail(LACX_E_DEVICE, std::string(what) + ": " + hipGetErrorString(_e));               \
            goto done;                                                                                       \
        }                                                                                                    \
    } while (0)
        const char* what = "";
        // the verify form of a WAV image in host memory (a batch of one): the data chunk behind the payload and its pad
        const uint8_t* host_src = verify && m == 1 ? in[dev[0]].host_src : nullptr;
        const uint64_t host_src_bytes = host_src ? in[dev[0]].host_src_bytes : 0;
        const uint64_t src_at = (total_pay + kDecodeTailPad + 15u) & ~15ull;  // 16-byte aligned: hipMalloc's base is
        hipStream_t st = to == DecodeTo::device || (verify && !host_src) ? stream : d->stream;
        const uint32_t T = (uint32_t)total_blocks;
        // LACX_DECODE_BATCH_PAD=1 (tuning knob, read per call): every item's blocks start a new wave
        const char* pad_env = std::getenv("LACX_DECODE_BATCH_PAD");
        const bool pad = pad_env && pad_env[0] == '1';
        std::vector<uint32_t> lane_blk, v2_items;
        lane_blk.reserve(v3_blocks);
        for (uint32_t j = 0; j < m; ++j) {
            if (it[j].version == 2) {
                v2_items.push_back(j);
                continue;
            }
            if (pad) while (lane_blk.size() % 64u) lane_blk.push_back(~0u);
            for (uint32_t b = 0; b < it[j].blocks; ++b) lane_blk.push_back(it[j].block0 + b);
        }
        // metadata, one upload: items | byte_off [T + 1] | frame_off [T + 1] | unit_off [m + 1] | blk_item [T] |
        // lane_blk | v2_items
        const size_t o_items = 0, o_byte = (sizeof(DecodeItem) * m + 15u) & ~(size_t)15u;
        const size_t o_frame = o_byte + 8 * ((size_t)T + 1), o_unit = o_frame + 8 * ((size_t)T + 1);
        const size_t o_bitem = o_unit + 8 * ((size_t)m + 1), o_lane = o_bitem + 4 * (size_t)T;
        const size_t o_v2 = o_lane + 4 * lane_blk.size(), o_win = (o_v2 + 4 * v2_items.size() + 15u) & ~(size_t)15u;
        const size_t o_res = o_win + sizeof(VerifySource) * m;  // verify form: | ver [m] | res [m] in the window form's place
        const size_t meta = verify ? o_res + sizeof(VerifyWords) * m
                                   : window >= 0 ? o_win + sizeof(WindowOut) * m : o_v2 + 4 * v2_items.size();  // | win [m]
        DEC_TRY(decoder_open(d, &prev_device, &what), what);
        if (host_src) st = d->stream;  // (created by decoder_open)
        DEC_TRY(grow_payload(d, host_src ? src_at + host_src_bytes : total_pay, &what), what);
        DEC_TRY(grow_blocks(d, T, &what), what);
        if (wav || (window >= 0 && to == DecodeTo::host)) DEC_TRY(grow_wav(d, image_total, &what), what);
        if (own_pcm) DEC_TRY(grow_pcm(d, pcm_total, &what), what);
        if (meta > d->meta_cap) {
            if (d->d_meta) (void)hipFree(d->d_meta);
            if (d->h_meta) (void)hipHostFree(d->h_meta);
            d->d_meta = d->h_meta = nullptr;
            d->meta_cap = 0;
            const uint64_t cap = meta + meta / 8 + 256;
            DEC_TRY(hipMalloc((void**)&d->d_meta, cap), "hipMalloc(batch tables)");
            DEC_TRY(hipHostMalloc((void**)&d->h_meta, cap, 0), "hipHostMalloc(batch tables)");
            d->meta_cap = cap;
        }
        {
            uint8_t* h = d->h_meta;
            auto* byte_off = reinterpret_cast<unsigned long long*>(h + o_byte);
            auto* frame_off = reinterpret_cast<unsigned long long*>(h + o_frame);
            auto* unit_off = reinterpret_cast<unsigned long long*>(h + o_unit);
            auto* blk_item = reinterpret_cast<uint32_t*>(h + o_bitem);
            byte_off[0] = frame_off[0] = unit_off[0] = 0;
            for (uint32_t j = 0; j < m; ++j) {
                const BatchIn& x = in[dev[j]];
                DecodeItem& y = it[j];
                const bool v2 = y.version == 2;
                const uint64_t entry = v2 ? 4u : 8u;
                for (uint32_t b = 0; b < y.blocks; ++b) {
                    const uint32_t g = y.block0 + b;
                    const uint64_t sb = blk_first[j] + b;  // the block within the stream
                    frame_off[g + 1] = frame_off[g] + be32(x.lac + 14 + entry * sb);
                    byte_off[g + 1] = v2 ? byte_off[g] : byte_off[g] + be32(x.lac + 18 + 8ull * sb);
                    blk_item[g] = j;
                }
                if (v2) {  // the version-2 item's bytes count in the byte offsets as one lump at its last block
                    byte_off[y.block0 + y.blocks] = y.pay_off + (y.pay_bits >> 3);
                }
                unit_off[j + 1] = unit_off[j] + (y.frames + 3u) / 4u;
                if (own_pcm) {
                    y.left = d->d_left + pcm_at[j];
                    y.right = y.channels == 2 ? d->d_right + pcm_at[j] : nullptr;
                }
                if (wav) y.wav = d->d_wav + wav_at[j];
                if (window >= 0 && to == DecodeTo::host) {
                    win[j].left = d->d_wav + win_at[j];
                    win[j].right = y.channels == 2 ? d->d_wav + win_at[j] + 4 * win[j].frames : nullptr;
                }
            }
            if (window >= 0) std::memcpy(h + o_win, win.data(), sizeof(WindowOut) * m);
            if (verify) {
                auto* ver = reinterpret_cast<VerifySource*>(h + o_win);
                auto* res = reinterpret_cast<VerifyWords*>(h + o_res);
                for (uint32_t j = 0; j < m; ++j) {
                    const lacx_pcm& p = in[dev[j]].pcm;
                    ver[j] = VerifySource{host_src ? d->d_pay + src_at : p.data0, p.data1, p.layout, 0};
                    res[j] = VerifyWords{0, ~0ull, 0, 0, 0, 0};
                }
            }
            std::memcpy(h + o_items, it.data(), sizeof(DecodeItem) * m);
            if (!lane_blk.empty()) std::memcpy(h + o_lane, lane_blk.data(), 4 * lane_blk.size());
            if (!v2_items.empty()) std::memcpy(h + o_v2, v2_items.data(), 4 * v2_items.size());
        }
        {
            DEC_TRY(hipMemcpyAsync(d->d_meta, d->h_meta, meta, hipMemcpyHostToDevice, st), "H2D batch tables");
            if (window >= 0) {  // the windows' ranges through the pinned stage: one copy
                DEC_TRY(grow_pay_stage(d, total_pay, &what), what);
                std::vector<const uint8_t*> src(m);
                std::vector<uint64_t> off(m);
                for (uint32_t j = 0; j < m; ++j) {
                    src[j] = in[dev[j]].lac + 14 + (info[dev[j]].version == 2 ? 4ull : 8ull) * info[dev[j]].blocks + pay_src[j];
                    off[j] = it[j].pay_off;
                }
                gather_ranges(d->h_pay, src, off, pay_bytes, total_pay);
                DEC_TRY(hipMemcpyAsync(d->d_pay, d->h_pay, total_pay, hipMemcpyHostToDevice, st), "H2D payload");
            } else {
                for (uint32_t j = 0; j < m; ++j) {
                    const BatchIn& x = in[dev[j]];
                    const uint64_t head = 14 + (it[j].version == 2 ? 4ull : 8ull) * it[j].blocks;
                    DEC_TRY(hipMemcpyAsync(d->d_pay + it[j].pay_off, x.lac + head, x.size - head, hipMemcpyHostToDevice, st), "H2D payload");
                }
            }
            DEC_TRY(hipMemsetAsync(d->d_pay + total_pay, 0, kDecodeTailPad, st), "memset");  // the bit reader's look-ahead
            if (host_src) DEC_TRY(hipMemcpyAsync(d->d_pay + src_at, host_src, host_src_bytes, hipMemcpyHostToDevice, st), "H2D source");
            DecodeArgs a;
            uint8_t* dm = d->d_meta;
            a.nitems = m;
            a.total_blocks = T;
            a.items = reinterpret_cast<const DecodeItem*>(dm + o_items);
            a.blk_item = reinterpret_cast<const uint32_t*>(dm + o_bitem);
            a.lanes = (uint32_t)lane_blk.size();
            a.lane_blk = reinterpret_cast<const uint32_t*>(dm + o_lane);
            a.nv2 = (uint32_t)v2_items.size();
            a.v2_items = reinterpret_cast<const uint32_t*>(dm + o_v2);
            a.payload = d->d_pay;
            a.byte_off = reinterpret_cast<const unsigned long long*>(dm + o_byte);
            a.frame_off = reinterpret_cast<const unsigned long long*>(dm + o_frame);
            a.status = d->d_status;
            a.ms_flag = d->d_ms;
            a.wav = wav;
            a.unit_off = reinterpret_cast<const unsigned long long*>(dm + o_unit);
            a.total_units = total_units;
            if (window >= 0) a.window = reinterpret_cast<const WindowOut*>(dm + o_win);
            a.f32 = window == LACX_SAMPLE_F32;
            if (verify) {
                a.verify = reinterpret_cast<const VerifySource*>(dm + o_win);
                a.verify_res = reinterpret_cast<VerifyWords*>(dm + o_res);
            }
            DEC_TRY(hipEventRecord(d->e0, st), "event record");
            DEC_TRY(launch_decode(a, st), "decode launch");
            DEC_TRY(hipEventRecord(d->e1, st), "event record");
            DEC_TRY(hipMemcpyAsync(d->h_status, d->d_status, (size_t)T * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H status");
            // the images of the items that decoded are valid whatever the others did: one copy for all
            if (wav) DEC_TRY(hipMemcpyAsync(d->h_wav, d->d_wav, image_total, hipMemcpyDeviceToHost, st), "D2H WAV images");
            // the verify form's whole answer: 32 bytes per item
            if (verify) DEC_TRY(hipMemcpyAsync(d->h_meta + o_res, d->d_meta + o_res, sizeof(VerifyWords) * m, hipMemcpyDeviceToHost, st), "D2H verify results");
            DEC_TRY(hipStreamSynchronize(st), "synchronize");
            if (device_ms) (void)hipEventElapsedTime(device_ms, d->e0, d->e1);
        }
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t i = dev[j];
            for (uint32_t b = 0; b < it[j].blocks; ++b) {
                const uint32_t sv = d->h_status[it[j].block0 + b];
                if (sv) {  // the item's first failing block, like the reference's message (lac/decoder.cpp:24-32)
                    code[i] = LACX_E_RUNTIME;
                    err[i] = "[decode-error] block=" + std::to_string(blk_first[j] + b) + " " + block_error(sv);
                    break;
                }
            }
            if (code[i] != LACX_OK) continue;
            if (verify) {
                const VerifyWords& w = reinterpret_cast<const VerifyWords*>(d->h_meta + o_res)[j];
                if (w.count == 0) continue;
                lacx_verify_result r{};
                r.mismatches = w.count;
                r.frame = w.key >> 1;
                r.block = w.block;
                r.channel = (uint8_t)(w.key & 1u);
                r.decoded = w.decoded;
                r.source = w.source;
                if (vres) vres[i] = r;
                code[i] = LACX_E_MISMATCH;
                err[i] = "[verify-error] block=" + std::to_string(r.block) + " channel=" + (r.channel ? "right" : "left") +
                         " frame=" + std::to_string(r.frame) + " decoded=" + std::to_string(r.decoded) +
                         " source=" + std::to_string(r.source) + " mismatches=" + std::to_string(r.mismatches);
                continue;
            }
            if (wav) {
                uint8_t* img = d->h_wav + wav_at[j];
                (void)wav_header(info[i], img);
                if (out) out[i] = lacx_span{img, image_size[j]};
            }
            if (to == DecodeTo::host && window >= 0) {
                const uint64_t bytes = win[j].frames * 4u;
                DEC_TRY(hipMemcpyAsync(in[i].left, win[j].left, bytes, hipMemcpyDeviceToHost, st), "D2H left");
                if (it[j].channels == 2) DEC_TRY(hipMemcpyAsync(in[i].right, win[j].right, bytes, hipMemcpyDeviceToHost, st), "D2H right");
            } else if (to == DecodeTo::host) {  // the two channels leave on two streams' worth of copy engine time: issue, then wait
                const uint64_t bytes = it[j].frames * sizeof(int32_t);
                DEC_TRY(hipMemcpyAsync(in[i].left, d->d_left + pcm_at[j], bytes, hipMemcpyDeviceToHost, st), "D2H left");
                if (it[j].channels == 2)
                    DEC_TRY(hipMemcpyAsync(in[i].right, d->d_right + pcm_at[j], bytes, hipMemcpyDeviceToHost, st), "D2H right");
            }
        }
        if (to == DecodeTo::host) DEC_TRY(hipStreamSynchronize(st), "synchronize");
#undef DEC_TRY
    }
done:
    if (prev_device >= 0) (void)hipSetDevice(prev_device);
    if (rc != LACX_OK) {  // the whole call failed: no item decoded
        for (uint32_t i = 0; i < n; ++i) {
            if (code[i] != LACX_OK) continue;
            code[i] = rc;
            err[i] = g_decode_err;
            if (out) out[i] = lacx_span{nullptr, 0};
        }
    }
    return rc;
}

// A batch entry point's result: the per-item outcome into item_rc and d->item_err, and the lowest failing item's code
// with "stream i: <message>" (or the whole call's failure).
int batch_result(lacx_decoder* d, int rc, const std::vector<int>& code, std::vector<std::string>& err, int* item_rc) {
    if (item_rc) std::copy(code.begin(), code.end(), item_rc);
    d->item_err = std::move(err);
    if (rc != LACX_OK) return rc;
    for (size_t i = 0; i < code.size(); ++i)
        if (code[i] != LACX_OK) return decode_fail(code[i], "stream " + std::to_string(i) + ": " + d->item_err[i]);
    return LACX_OK;
}

// A single stream as a batch of one: its own code and message.  d->item_err keeps the last batch call's.
int decode_one(lacx_decoder* d, const BatchIn& in, DecodeTo to, lacx_span* out, float* device_ms, int window = -1) {
    std::vector<int> code;
    std::vector<std::string> err;
    (void)decode_batch_run(d, &in, 1, to, nullptr, out, code, err, device_ms, window);
    return code[0] == LACX_OK ? LACX_OK : decode_fail(code[0], err[0]);
}
}  // namespace

int lacx_decoder_decode(lacx_decoder* d, const uint8_t* lac, uint64_t size, int32_t* left, int32_t* right, uint64_t frames,
                        float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    return decode_one(d, BatchIn{lac, size, left, right, frames}, DecodeTo::host, nullptr, device_ms);
}

int lacx_decoder_decode_wav_view(lacx_decoder* d, const uint8_t* lac, uint64_t size, const uint8_t** out, uint64_t* out_size,
                                 float* device_ms) {
    if (out) *out = nullptr;
    if (out_size) *out_size = 0;
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!out || !out_size) return decode_fail(LACX_E_INVALID, "null argument");
    lacx_span img{nullptr, 0};
    const int rc = decode_one(d, BatchIn{lac, size, nullptr, nullptr, 0}, DecodeTo::wav, &img, device_ms);
    if (rc) return rc;
    *out = img.data;  // the start of d->h_wav: a batch of one
    *out_size = img.size;
    return LACX_OK;
}

int lacx_decoder_decode_wav(lacx_decoder* d, const uint8_t* lac, uint64_t size, uint8_t** out, uint64_t* out_size,
                            float* device_ms) {
    if (out) *out = nullptr;
    if (out_size) *out_size = 0;
    if (!out || !out_size) return decode_fail(LACX_E_INVALID, "null argument");
    const uint8_t* view = nullptr;
    uint64_t n = 0;
    const int rc = lacx_decoder_decode_wav_view(d, lac, size, &view, &n, device_ms);
    if (rc) return rc;
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(n));
    if (!buf) return decode_fail(LACX_E_RUNTIME, "out of host memory");
    std::memcpy(buf, view, n);
    *out = buf;
    *out_size = n;
    return LACX_OK;
}

int lacx_decoder_decode_wav_batch_view(lacx_decoder* d, const lacx_span* lacs, uint32_t n, lacx_span* out, int* item_rc,
                                       float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || !out || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i].data, lacs[i].size, nullptr, nullptr, 0};
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = decode_batch_run(d, in.data(), n, DecodeTo::wav, nullptr, out, code, err, device_ms);
    return batch_result(d, rc, code, err, item_rc);
}

int lacx_decoder_decode_wav_batch(lacx_decoder* d, const lacx_span* lacs, uint32_t n, lacx_span* out, int* item_rc,
                                  float* device_ms) {
    const int rc = lacx_decoder_decode_wav_batch_view(d, lacs, n, out, item_rc, device_ms);
    if (!out || !lacs || n == 0 || !d) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        if (!out[i].data) continue;
        uint8_t* buf = static_cast<uint8_t*>(std::malloc(out[i].size));
        if (!buf) {
            for (uint32_t k = 0; k < i; ++k) {
                std::free(const_cast<uint8_t*>(out[k].data));
                out[k] = lacx_span{nullptr, 0};
            }
            for (uint32_t k = i; k < n; ++k) out[k] = lacx_span{nullptr, 0};
            return decode_fail(LACX_E_RUNTIME, "out of host memory");
        }
        std::memcpy(buf, out[i].data, out[i].size);
        out[i].data = buf;
    }
    return rc;
}

int lacx_decoder_decode_batch_device(lacx_decoder* d, const lacx_decode_item* items, uint32_t n, void* stream, int* item_rc,
                                     float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!items || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{items[i].lac, items[i].size, items[i].left, items[i].right, items[i].frames};
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = decode_batch_run(d, in.data(), n, DecodeTo::device, static_cast<hipStream_t>(stream), nullptr, code, err,
                                    device_ms);
    return batch_result(d, rc, code, err, item_rc);
}

int lacx_decoder_decode_window_batch_device(lacx_decoder* d, const lacx_window_item* items, uint32_t n, int sample_type,
                                            void* stream, int* item_rc, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!items || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    if (sample_type != LACX_SAMPLE_I32 && sample_type != LACX_SAMPLE_F32) return decode_fail(LACX_E_INVALID, "unknown sample type");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i)
        in[i] = BatchIn{items[i].lac, items[i].size, static_cast<int32_t*>(items[i].left), static_cast<int32_t*>(items[i].right),
                        items[i].frames, items[i].start};
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = decode_batch_run(d, in.data(), n, DecodeTo::device, static_cast<hipStream_t>(stream), nullptr, code, err,
                                    device_ms, sample_type);
    return batch_result(d, rc, code, err, item_rc);
}

int lacx_decoder_decode_window(lacx_decoder* d, const uint8_t* lac, uint64_t size, uint64_t start, uint64_t frames,
                               int sample_type, void* left, void* right, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (sample_type != LACX_SAMPLE_I32 && sample_type != LACX_SAMPLE_F32) return decode_fail(LACX_E_INVALID, "unknown sample type");
    return decode_one(d, BatchIn{lac, size, static_cast<int32_t*>(left), static_cast<int32_t*>(right), frames, start},
                      DecodeTo::host, nullptr, device_ms, sample_type);
}

int lacx_decoder_verify_batch_device(lacx_decoder* d, const lacx_verify_item* items, uint32_t n, void* stream, int* item_rc,
                                     lacx_verify_result* results, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!items || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) {
        in[i] = BatchIn{items[i].lac, items[i].size, nullptr, nullptr, items[i].frames};
        in[i].pcm = items[i].pcm;
    }
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = decode_batch_run(d, in.data(), n, DecodeTo::verify, static_cast<hipStream_t>(stream), nullptr, code, err,
                                    device_ms, -1, results);
    return batch_result(d, rc, code, err, item_rc);
}

// A WAV file image in host memory against a stream: the formats are compared on the host (a difference is an answer
// that needs no device), then the data chunk goes to the device as it is, 2 or 3 bytes per sample, and is compared
// there as an interleaved source -- a batch of one.  No PCM comes back.
int lacx_decoder_verify_wav(lacx_decoder* d, const uint8_t* lac, uint64_t size, const uint8_t* wav, uint64_t wav_size,
                            lacx_verify_result* result, float* device_ms) {
    if (device_ms) *device_ms = 0.f;
    if (result) std::memset(result, 0, sizeof(*result));
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!wav) return decode_fail(LACX_E_INVALID, "null argument");
    lacx_stream_info info;
    const int prc = lacx_stream_parse(lac, size, &info);
    if (prc != LACX_OK) return prc;
    lacx_wav_info w;
    if (lacx_wav_parse(wav, wav_size, &w) != LACX_OK) return decode_fail(LACX_E_INVALID, "[verify-error] source is not a PCM WAV file the encoder reads");
    auto differs = [](const char* field, uint64_t a, uint64_t b) {
        return decode_fail(LACX_E_MISMATCH, std::string("[verify-error] ") + field + ": stream " + std::to_string(a) + ", source " + std::to_string(b));
    };
    if (w.channels != info.channels) return differs("channels", info.channels, w.channels);
    if (w.bit_depth != info.bit_depth) return differs("bit depth", info.bit_depth, w.bit_depth);
    if (w.sample_rate != info.sample_rate) return differs("sample rate", info.sample_rate, w.sample_rate);
    if (w.frames != info.frames) return differs("frames", info.frames, w.frames);
    BatchIn in{lac, size, nullptr, nullptr, w.frames};
    in.pcm = lacx_pcm{nullptr, nullptr, w.bit_depth == 16 ? LACX_PCM_INTERLEAVED_I16 : LACX_PCM_INTERLEAVED_I24, w.channels};
    in.host_src = wav + w.data_offset;
    in.host_src_bytes = w.frames * w.channels * (uint64_t)(w.bit_depth / 8);
    std::vector<int> code;
    std::vector<std::string> err;
    (void)decode_batch_run(d, &in, 1, DecodeTo::verify, nullptr, nullptr, code, err, device_ms, -1, result);
    return code[0] == LACX_OK ? LACX_OK : decode_fail(code[0], err[0]);
}

const char* lacx_decoder_item_error(const lacx_decoder* d, uint32_t i) {
    if (!d || i >= d->item_err.size()) return "";
    return d->item_err[i].c_str();
}

int lacx_decode(int device, const uint8_t* lac, uint64_t size, int32_t* left, int32_t* right, uint64_t frames,
                float* device_ms) {
    int dev = device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = -1;
    if (dev < 0 || dev >= kMaxDecodeDevices) {
        if (lacx_device_count() <= 0) {  // (parse errors come first, as before)
            lacx_stream_info info;
            const int prc = lacx_stream_parse(lac, size, &info);
            return prc ? prc : decode_fail(LACX_E_DEVICE, "no usable HIP device");
        }
        return decode_fail(LACX_E_DEVICE, "HIP device ordinal out of range");
    }
    SharedDecoder* sd = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_shared_mu);
        if (!g_shared[dev]) {
            g_shared[dev] = new SharedDecoder();
            g_shared[dev]->dec.device = dev;
        }
        sd = g_shared[dev];
    }
    std::lock_guard<std::mutex> lock(sd->mu);
    lacx_decoder* d = &sd->dec;
    return lacx_decoder_decode(d, lac, size, left, right, frames, device_ms);
}

}  // extern "C"
