// api_decode.cpp -- the decode entry points of the C ABI: container parsing and the device decoder's host side.
#include "decode_plan.h"
#include "device_buf.h"
#include "encoder_impl.h"

// (the entry points are declared extern "C" in lacx.h)
// ---- decode -------------------------------------------------------------------------------------
namespace {
thread_local std::string g_decode_err;
int decode_fail(int code, const std::string& msg) {
    g_decode_err = msg;
    return code;
}
}  // namespace

const char* lacx_decode_last_error(void) { return g_decode_err.c_str(); }

int lacx_stream_parse(const uint8_t* lac, uint64_t size, lacx_stream_info* out) {  // the container walk: decode_plan.h
    const char* why = "";
    const int c = parse_stream(lac, size, out, &why);
    return c == LACX_OK ? c : decode_fail(c, why);
}

// The decoder object: device buffers, a stream and two events that live from call to call (grow-only), so that a decode
// costs its copies and its kernel, not six allocations (ref LAC::Decoder is an object too, src/codec/lac/decoder.hpp:10-24).
struct lacx_decoder {
    int device = -1;  // -1: whatever device is current at the first call
    bool ready = false;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    Buf pay{{{false, 1, "hipMalloc(payload)"}}};
    Buf stage{{{true, 1, "hipHostMalloc(payload stage)"}}};  // the window form's payload ranges, gathered for one H2D copy
    Buf pcm{{{false, 4, "hipMalloc(left)"}, {false, 4, "hipMalloc(right)"}}};  // both channels, whatever the streams' count
    Buf blocks{{{false, 4, "hipMalloc(status)"}, {false, 1, "hipMalloc(flags)"}, {true, 4, "hipHostMalloc(status)"}}};
    Buf image{{{false, 1, "hipMalloc(wav)"}, {true, 1, "hipHostMalloc(wav)"}}};  // WAV images (header + data + pad), host windows
    Buf tables{{{false, 1, "hipMalloc(batch tables)"}, {true, 1, "hipHostMalloc(batch tables)"}}};  // one upload (TableLayout)
    uint8_t* d_pay() const { return static_cast<uint8_t*>(pay.part[0].p); }
    uint8_t* h_pay() const { return static_cast<uint8_t*>(stage.part[0].p); }
    int32_t* d_left() const { return static_cast<int32_t*>(pcm.part[0].p); }
    int32_t* d_right() const { return static_cast<int32_t*>(pcm.part[1].p); }
    uint32_t* d_status() const { return static_cast<uint32_t*>(blocks.part[0].p); }
    uint8_t* d_ms() const { return static_cast<uint8_t*>(blocks.part[1].p); }
    uint32_t* h_status() const { return static_cast<uint32_t*>(blocks.part[2].p); }
    uint8_t* d_wav() const { return static_cast<uint8_t*>(image.part[0].p); }
    uint8_t* h_wav() const { return static_cast<uint8_t*>(image.part[1].p); }  // behind lacx_decoder_decode_wav_view
    uint8_t* d_meta() const { return static_cast<uint8_t*>(tables.part[0].p); }
    uint8_t* h_meta() const { return static_cast<uint8_t*>(tables.part[1].p); }
    std::vector<std::string> item_err;  // the last batch call's message per item ("" = decoded)
    std::string err;
};

namespace {
void decoder_release(lacx_decoder* d) {
    if (d->ready) (void)hipSetDevice(d->device);
    if (d->e0) (void)hipEventDestroy(d->e0);
    if (d->e1) (void)hipEventDestroy(d->e1);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    for (Buf* b : {&d->pay, &d->stage, &d->pcm, &d->blocks, &d->image, &d->tables}) buf_free(*b);
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
// The 44-byte canonical header of the decoded WAV (ref src/main.cpp:127-148, 248-262).
void wav_header(const lacx_stream_info& info, uint8_t* h) {
    const uint32_t align = (uint32_t)info.channels * (info.bit_depth / 8u);
    const uint64_t data = info.frames * align, pad = data & 1u;
    auto u16 = [&](int at, uint32_t v) { h[at] = (uint8_t)v, h[at + 1] = (uint8_t)(v >> 8); };
    auto u32 = [&](int at, uint32_t v) { u16(at, v & 0xFFFFu), u16(at + 2, v >> 16); };
    std::memcpy(h, "RIFF", 4);
    u32(4, (uint32_t)(36u + data + pad));  // below 2^32: parse_stream's RIFF limit
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
}

const char* block_error(uint32_t st) {
    static const char* const kWhat[] = {"", "block header", "channel header", "residual", "padding", "sample overflow",
                                        "trailing bytes", "sample outside the bit depth", "not reached", "residual beyond 2^30"};
    return st < 10 ? kWhat[st] : "?";
}

// A decode job: the items (BatchIn, DecodeForm, sample type: decode_plan.h) and where the call's answers go.
struct DecodeJob {
    const BatchIn* in;
    uint32_t n;
    DecodeForm form;
    int sample_type = kWholeStreams;
    hipStream_t stream = nullptr;        // the caller's: device form, verify form against device PCM
    lacx_span* out = nullptr;            // wav form: [n] each item's image in the decoder's pinned image buffer
    lacx_verify_result* vres = nullptr;  // verify form: [n]
    float* device_ms = nullptr;
};

// ---- the steps of a run (decode_batch_run) ----
DevErr decoder_open(lacx_decoder* d, int* prev_device) {  // *prev_device: to put back, or -1
    *prev_device = -1;
    if (!d->ready && d->device < 0)
        if (DevErr e = chk(hipGetDevice(&d->device), "hipGetDevice")) return e;
    int cur = -1;
    if (DevErr e = chk(hipGetDevice(&cur), "hipGetDevice")) return e;
    if (cur != d->device) {
        if (DevErr e = chk(hipSetDevice(d->device), "hipSetDevice")) return e;
        *prev_device = cur;
    }
    if (!d->ready) {
        if (DevErr e = chk(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking), "hipStreamCreate")) return e;
        if (DevErr e = chk(hipEventCreate(&d->e0), "hipEventCreate")) return e;
        if (DevErr e = chk(hipEventCreate(&d->e1), "hipEventCreate")) return e;
        d->ready = true;
    }
    return DevErr{};
}

// The plan's capacities, each buffer with its own slack: the image buffer and the PCM buffers grow to what is asked.
DevErr ensure_capacities(lacx_decoder* d, const DecodePlan& plan) {
    const auto& need = plan.need;
    const struct {
        Buf& buf;
        uint64_t need, slack;
    } want[] = {{d->pay, need.payload, (need.payload - kDecodeTailPad) / 8},
                {d->blocks, need.blocks, need.blocks / 8 + 16},
                {d->image, need.image, 0},
                {d->pcm, need.pcm_frames, 0},
                {d->tables, need.tables, need.tables / 8 + 256},
                {d->stage, need.stage, need.stage / 8 + 4096}};
    for (const auto& w : want)
        if (w.need)
            if (DevErr e = buf_grow(w.buf, w.need, w.slack)) return e;
    return DevErr{};
}

DevErr upload_tables(lacx_decoder* d, const DecodeJob& job, const DecodePlan& plan, hipStream_t st) {
    plan_fill_tables(plan, job.in, PlanBases{d->d_pay(), d->d_left(), d->d_right(), d->d_wav()}, d->h_meta());
    return chk(hipMemcpyAsync(d->d_meta(), d->h_meta(), plan.at.size, hipMemcpyHostToDevice, st), "H2D batch tables");
}

// dst[pay_off, pay_off + pay_bytes) = every item's payload range, the destination split into equal byte ranges over up to
// 8 threads (the calling thread takes the first): a window batch is many short ranges of different streams, which as
// one pageable copy each would cost 10-20 us apiece in the runtime.
void gather_ranges(uint8_t* dst, const DecodePlan& plan, const BatchIn* in) {
    const uint64_t total = plan.total_pay;
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned nt = total < (8u << 20) ? 1u : std::max(1u, std::min(8u, hw));
    auto part = [&](unsigned t) {
        const uint64_t lo = total * t / nt, hi = total * (t + 1) / nt;
        for (const PlanItem& p : plan.items) {
            const uint64_t off = p.item.pay_off, a = std::max(lo, off), b = std::min(hi, off + p.pay_bytes);
            if (a < b) std::memcpy(dst + a, in[p.src].lac + p.head + p.pay_src + (a - off), b - a);
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

DevErr upload_payload(lacx_decoder* d, const DecodeJob& job, const DecodePlan& plan, hipStream_t st) {
    if (plan.window()) {  // the windows' ranges through the pinned stage: one copy
        gather_ranges(d->h_pay(), plan, job.in);
        if (DevErr e = chk(hipMemcpyAsync(d->d_pay(), d->h_pay(), plan.total_pay, hipMemcpyHostToDevice, st), "H2D payload")) return e;
    } else {
        for (const PlanItem& p : plan.items)
            if (DevErr e = chk(hipMemcpyAsync(d->d_pay() + p.item.pay_off, job.in[p.src].lac + p.head, p.pay_bytes, hipMemcpyHostToDevice, st),
                               "H2D payload"))
                return e;
    }
    if (DevErr e = chk(hipMemsetAsync(d->d_pay() + plan.total_pay, 0, kDecodeTailPad, st), "memset")) return e;  // the bit reader's look-ahead
    if (!plan.host_src) return DevErr{};
    return chk(hipMemcpyAsync(d->d_pay() + plan.src_at, plan.host_src, plan.host_src_bytes, hipMemcpyHostToDevice, st), "H2D source");
}

// The kernels between the decoder's two events, then what every form reads back, and the wait for it.
DevErr launch_and_wait(lacx_decoder* d, const DecodeJob& job, const DecodePlan& plan, hipStream_t st) {
    const DecodeArgs a = plan_args(plan, d->d_meta(), d->d_pay(), d->d_status(), d->d_ms());
    const size_t res = plan.at.res, m = plan.items.size();
    if (DevErr e = chk(hipEventRecord(d->e0, st), "event record")) return e;
    if (DevErr e = chk(launch_decode(a, st), "decode launch")) return e;
    if (DevErr e = chk(hipEventRecord(d->e1, st), "event record")) return e;
    if (DevErr e = chk(hipMemcpyAsync(d->h_status(), d->d_status(), (size_t)plan.total_blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H status"))
        return e;
    // the images of the items that decoded are valid whatever the others did: one copy for all
    if (plan.form == DecodeForm::wav)
        if (DevErr e = chk(hipMemcpyAsync(d->h_wav(), d->d_wav(), plan.image_total, hipMemcpyDeviceToHost, st), "D2H WAV images")) return e;
    // the verify form's whole answer: 32 bytes per item
    if (plan.form == DecodeForm::verify)
        if (DevErr e = chk(hipMemcpyAsync(d->h_meta() + res, d->d_meta() + res, sizeof(VerifyWords) * m, hipMemcpyDeviceToHost, st), "D2H verify results"))
            return e;
    if (DevErr e = chk(hipStreamSynchronize(st), "synchronize")) return e;
    if (job.device_ms) (void)hipEventElapsedTime(job.device_ms, d->e0, d->e1);
    return DevErr{};
}

// Per item: its first failing block, else what its form gives back.
DevErr collect(lacx_decoder* d, const DecodeJob& job, const DecodePlan& plan, hipStream_t st, std::vector<int>& code,
               std::vector<std::string>& err) {
    const bool host = plan.form == DecodeForm::host;
    for (size_t j = 0; j < plan.items.size(); ++j) {
        const PlanItem& p = plan.items[j];
        const BatchIn& x = job.in[p.src];
        const uint32_t i = p.src;
        for (uint32_t b = 0; b < p.item.blocks; ++b) {
            const uint32_t sv = d->h_status()[p.item.block0 + b];
            if (sv) {  // the item's first failing block, like the reference's message (lac/decoder.cpp:24-32)
                code[i] = LACX_E_RUNTIME;
                err[i] = "[decode-error] block=" + std::to_string(p.blk_first + b) + " " + block_error(sv);
                break;
            }
        }
        if (code[i] != LACX_OK) continue;
        if (plan.form == DecodeForm::verify) {
            const VerifyWords& w = reinterpret_cast<const VerifyWords*>(d->h_meta() + plan.at.res)[j];
            if (w.count == 0) continue;
            lacx_verify_result r{};
            r.mismatches = w.count;
            r.frame = w.key >> 1;
            r.block = w.block;
            r.channel = (uint8_t)(w.key & 1u);
            r.decoded = w.decoded;
            r.source = w.source;
            if (job.vres) job.vres[i] = r;
            code[i] = LACX_E_MISMATCH;
            err[i] = "[verify-error] block=" + std::to_string(r.block) + " channel=" + (r.channel ? "right" : "left") +
                     " frame=" + std::to_string(r.frame) + " decoded=" + std::to_string(r.decoded) +
                     " source=" + std::to_string(r.source) + " mismatches=" + std::to_string(r.mismatches);
        } else if (plan.form == DecodeForm::wav) {
            uint8_t* img = d->h_wav() + p.image_at;
            wav_header(p.info, img);
            if (job.out) job.out[i] = lacx_span{img, p.image_size};
        } else if (host) {  // the two channels leave on two streams' worth of copy engine time: issue, then wait
            const uint64_t bytes = 4 * (plan.window() ? p.win.frames : p.item.frames);
            const uint8_t* stage = d->d_wav() + p.image_at;  // a window's samples: left, then right
            const void* left = plan.window() ? (const void*)stage : d->d_left() + p.pcm_at;
            const void* right = plan.window() ? (const void*)(stage + bytes) : d->d_right() + p.pcm_at;
            if (DevErr e = chk(hipMemcpyAsync(x.left, left, bytes, hipMemcpyDeviceToHost, st), "D2H left")) return e;
            if (p.item.channels == 2)
                if (DevErr e = chk(hipMemcpyAsync(x.right, right, bytes, hipMemcpyDeviceToHost, st), "D2H right")) return e;
        }
    }
    return host ? chk(hipStreamSynchronize(st), "synchronize") : DevErr{};
}

// The decoder: n streams as one decode (a single stream is n = 1), planned on the host (plan_decode: the per-item checks,
// the layout), then run as one device job.  Per item, code[i] and err[i] ("" = decoded): the message its decode gives.
// Returns LACX_OK, or LACX_E_DEVICE for a failure of the whole call (every item that passed its checks then carries it).
// The caller decides what the outcome becomes: the batch entry points keep it in d->item_err.
int decode_batch_run(lacx_decoder* d, const DecodeJob& job, std::vector<int>& code, std::vector<std::string>& err) {
    if (job.device_ms) *job.device_ms = 0.f;
    if (job.vres) std::memset(job.vres, 0, sizeof(lacx_verify_result) * job.n);
    // LACX_DECODE_BATCH_PAD=1 (tuning knob, read per call): every item's blocks start a new wave
    const char* pad_env = std::getenv("LACX_DECODE_BATCH_PAD");
    DecodePlan plan;
    const char* whole = plan_decode(job.in, job.n, job.form, job.sample_type, pad_env && pad_env[0] == '1', plan, code, err);
    if (lacx_device_count() <= 0) whole = "no usable HIP device";
    int rc = whole ? decode_fail(LACX_E_DEVICE, whole) : LACX_OK;
    if (!whole && !plan.items.empty()) {
        int prev_device = -1;
        DevErr e = decoder_open(d, &prev_device);
        // (d->stream: created by decoder_open)
        hipStream_t st = job.form == DecodeForm::device || (job.form == DecodeForm::verify && !plan.host_src) ? job.stream : d->stream;
        if (!e) e = ensure_capacities(d, plan);
        if (!e) e = upload_tables(d, job, plan, st);
        if (!e) e = upload_payload(d, job, plan, st);
        if (!e) e = launch_and_wait(d, job, plan, st);
        if (!e) e = collect(d, job, plan, st, code, err);
        if (prev_device >= 0) (void)hipSetDevice(prev_device);
        if (e) rc = decode_fail(LACX_E_DEVICE, std::string(e.what) + ": " + hipGetErrorString(e.e));
    }
    if (rc != LACX_OK) {  // the whole call failed: no item decoded
        for (uint32_t i = 0; i < job.n; ++i) {
            if (code[i] != LACX_OK) continue;
            code[i] = rc;
            err[i] = g_decode_err;
        }
    }
    for (uint32_t i = 0; job.out && i < job.n; ++i)
        if (code[i] != LACX_OK) job.out[i] = lacx_span{nullptr, 0};
    return rc;
}

// A batch entry point: runs the job; the per-item outcome into item_rc and d->item_err, and back the lowest failing item's
// code with "stream i: <message>" (or the whole call's failure).
int run_batch(lacx_decoder* d, const DecodeJob& job, int* item_rc) {
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = decode_batch_run(d, job, code, err);
    if (item_rc) std::copy(code.begin(), code.end(), item_rc);
    d->item_err = std::move(err);
    if (rc != LACX_OK) return rc;
    for (size_t i = 0; i < code.size(); ++i)
        if (code[i] != LACX_OK) return decode_fail(code[i], "stream " + std::to_string(i) + ": " + d->item_err[i]);
    return LACX_OK;
}

// A single stream as a batch of one: its own code and message.  d->item_err keeps the last batch call's.
int run_one(lacx_decoder* d, const BatchIn& in, DecodeJob job) {
    job.in = &in;
    job.n = 1;
    std::vector<int> code;
    std::vector<std::string> err;
    (void)decode_batch_run(d, job, code, err);
    return code[0] == LACX_OK ? LACX_OK : decode_fail(code[0], err[0]);
}
}  // namespace

int lacx_decoder_decode(lacx_decoder* d, const uint8_t* lac, uint64_t size, int32_t* left, int32_t* right, uint64_t frames,
                        float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    return run_one(d, BatchIn{lac, size, left, right, frames}, DecodeJob{nullptr, 1, DecodeForm::host, kWholeStreams, nullptr, nullptr, nullptr, device_ms});
}

int lacx_decoder_decode_wav_view(lacx_decoder* d, const uint8_t* lac, uint64_t size, const uint8_t** out, uint64_t* out_size,
                                 float* device_ms) {
    if (out) *out = nullptr;
    if (out_size) *out_size = 0;
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!out || !out_size) return decode_fail(LACX_E_INVALID, "null argument");
    lacx_span img{nullptr, 0};
    const int rc = run_one(d, BatchIn{lac, size, nullptr, nullptr, 0}, DecodeJob{nullptr, 1, DecodeForm::wav, kWholeStreams, nullptr, &img, nullptr, device_ms});
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
    return run_batch(d, DecodeJob{in.data(), n, DecodeForm::wav, kWholeStreams, nullptr, out, nullptr, device_ms}, item_rc);
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
    return run_batch(d, DecodeJob{in.data(), n, DecodeForm::device, kWholeStreams, static_cast<hipStream_t>(stream), nullptr, nullptr, device_ms}, item_rc);
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
    return run_batch(d, DecodeJob{in.data(), n, DecodeForm::device, sample_type, static_cast<hipStream_t>(stream), nullptr, nullptr, device_ms}, item_rc);
}

int lacx_decoder_decode_window(lacx_decoder* d, const uint8_t* lac, uint64_t size, uint64_t start, uint64_t frames,
                               int sample_type, void* left, void* right, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (sample_type != LACX_SAMPLE_I32 && sample_type != LACX_SAMPLE_F32) return decode_fail(LACX_E_INVALID, "unknown sample type");
    return run_one(d, BatchIn{lac, size, static_cast<int32_t*>(left), static_cast<int32_t*>(right), frames, start},
                   DecodeJob{nullptr, 1, DecodeForm::host, sample_type, nullptr, nullptr, nullptr, device_ms});
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
    return run_batch(d, DecodeJob{in.data(), n, DecodeForm::verify, kWholeStreams, static_cast<hipStream_t>(stream), nullptr, results, device_ms}, item_rc);
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
    return run_one(d, in, DecodeJob{nullptr, 1, DecodeForm::verify, kWholeStreams, nullptr, nullptr, result, device_ms});
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
