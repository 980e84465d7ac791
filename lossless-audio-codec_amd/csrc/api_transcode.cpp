// api_transcode.cpp -- lacx_transcode_batch: .lac in, .lac out (lacx.h).  Many outputs as one job, each a list of frame
// ranges of source streams, optionally re-channelled and re-quantised losslessly.  The job is planned on the host
// (edit_plan.h) and runs in two phases with one host look at the statuses between them.  Phase 1, on the decoder: one
// window job in the device form whose items' arrays point into the decoder's planar int32 staging (the splice costs no
// pass of its own), then k_edit (k_edit.hip) over all outputs, then the PCM digest kernel over what k_edit wrote.  Phase 2:
// lacx_encode_batch_device over the outputs that survived, lacx_assemble per output and, where asked for, the verify form
// with k_edit's buffer as its source.  The PCM never leaves the device.
#include "decoder_impl.h"
#include "edit_plan.h"
#include "encoder_impl.h"

namespace {

// The job between the host plan and the outcome; everything the phases hand on to each other.
struct Transcode {
    lacx_decoder* d;
    lacx_encoder* enc;
    const lacx_edit_segment* segs;
    uint32_t flags;
    const EditPlan& plan;
    std::vector<int>& code;          // per output of the call
    std::vector<std::string>& err;
    lacx_span* out;
    lacx_edit_result* results;       // nullable
    float ms = 0.f;
    bool alive(size_t j) const { return code[plan.outs[j].src] == LACX_OK; }
    lacx_pcm pcm(size_t j) const {
        const EditOut& e = plan.outs[j];
        return lacx_pcm{d->edit_dst.as<uint8_t>() + e.dst_at, nullptr, e.bit_depth == 16 ? LACX_PCM_INTERLEAVED_I16 : LACX_PCM_INTERLEAVED_I24, e.channels};
    }
};

int device_fail(const DevErr& e) { return decode_fail(LACX_E_DEVICE, std::string(e.what) + ": " + hipGetErrorString(e.e)); }

// Phase 1a: every segment a window item into the staging.  A segment that fails fails its output (the lowest one's words).
int decode_segments(Transcode& t) {
    const EditPlan& plan = t.plan;
    int32_t* stage = t.d->edit_stage.as<int32_t>();
    std::vector<lacx_window_item> items(plan.windows.size());
    for (size_t w = 0; w < items.size(); ++w) {
        const EditWindow& x = plan.windows[w];
        const EditOut& e = plan.outs[x.out];
        const lacx_edit_segment& s = t.segs[x.seg];
        items[w] = lacx_window_item{s.lac, s.size, x.start, x.frames, stage + e.stage_left + x.at, x.channels == 2 ? stage + e.stage_right + x.at : nullptr};
    }
    std::vector<int> wrc(items.size(), LACX_OK);
    float ms = 0.f;
    const int rc = lacx_decoder_decode_window_batch_device(t.d, items.data(), (uint32_t)items.size(), LACX_SAMPLE_I32, t.d->stream, wrc.data(), &ms);
    t.ms += ms;
    if (rc == LACX_E_DEVICE) return rc;
    for (size_t w = 0; w < items.size(); ++w) {
        const uint32_t i = plan.outs[plan.windows[w].out].src;
        if (wrc[w] == LACX_OK || t.code[i] != LACX_OK) continue;
        t.code[i] = wrc[w];
        t.err[i] = "segment " + std::to_string(plan.windows[w].k) + ": " + lacx_decoder_item_error(t.d, (uint32_t)w);
    }
    return LACX_OK;
}

// Phase 1b: k_edit over every planned output (the rows of one whose segments failed hold unspecified samples and its
// outcome is not looked at).  Tables: bad [m] | items [m] | unit_off [m + 1], one upload; 8 bytes per output back.
int edit_outputs(Transcode& t) {
    lacx_decoder* d = t.d;
    const EditPlan& plan = t.plan;
    const size_t m = plan.outs.size();
    const size_t at_items = (size_t)edit_detail::up(m * sizeof(EditBad), 16), at_off = at_items + (size_t)edit_detail::up(m * sizeof(EditItem), 16), size = at_off + 8 * (m + 1);
    if (DevErr e = buf_grow(d->edit_tab, size, size / 8 + 256)) return device_fail(e);
    uint8_t* h = d->edit_tab.as<uint8_t>(1);
    uint8_t* g = d->edit_tab.as<uint8_t>(0);
    std::memset(h, 0xFF, m * sizeof(EditBad));
    edit_fill_items(plan, d->edit_stage.as<int32_t>(), d->edit_dst.as<uint8_t>(), reinterpret_cast<EditItem*>(h + at_items));
    std::memcpy(h + at_off, plan.unit_off.data(), 8 * (m + 1));
    EditJob job{reinterpret_cast<const EditItem*>(g + at_items), reinterpret_cast<const unsigned long long*>(g + at_off), (uint32_t)m, 0, plan.unit_off.back()};
    hipStream_t st = d->stream;
    DevErr e = chk(hipMemcpyAsync(g, h, size, hipMemcpyHostToDevice, st), "H2D edit tables");
    if (!e) e = chk(hipEventRecord(d->e0, st), "event record");
    if (!e) e = chk(launch_edit(job, reinterpret_cast<EditBad*>(g), st), "edit launch");
    if (!e) e = chk(hipEventRecord(d->e1, st), "event record");
    if (!e) e = chk(hipMemcpyAsync(h, g, m * sizeof(EditBad), hipMemcpyDeviceToHost, st), "D2H edit result");
    if (!e) e = chk(hipStreamSynchronize(st), "synchronize");
    if (e) return device_fail(e);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, d->e0, d->e1);
    t.ms += ms;
    for (size_t j = 0; j < m; ++j) {
        const unsigned long long key = reinterpret_cast<const EditBad*>(h)[j].key;
        if (!t.alive(j) || key == kEditClean) continue;
        const EditOut& o = plan.outs[j];
        int32_t sl = 0, sr = 0;  // the value words: the staged samples of the frame
        const int32_t* stage = d->edit_stage.as<int32_t>();
        e = chk(hipMemcpy(&sl, stage + o.stage_left + (key >> 2), 4, hipMemcpyDeviceToHost), "D2H edit value");
        if (!e && o.src_channels == 2) e = chk(hipMemcpy(&sr, stage + o.stage_right + (key >> 2), 4, hipMemcpyDeviceToHost), "D2H edit value");
        if (e) return device_fail(e);
        t.code[o.src] = LACX_E_INVALID;
        t.err[o.src] = edit_bad_message(key, o.channel_op, sl, sr);
    }
    return LACX_OK;
}

// Phase 1c: the digest of what k_edit wrote, as the digest form's source PCM.
int digest_outputs(Transcode& t, const std::vector<size_t>& live, std::vector<lacx_digest>& dg) {
    std::vector<lacx_digest_source> src(live.size());
    for (size_t a = 0; a < live.size(); ++a) {
        const EditOut& e = t.plan.outs[live[a]];
        src[a] = lacx_digest_source{t.pcm(live[a]), e.frames, e.sample_rate, e.bit_depth, {0, 0, 0}};
    }
    dg.assign(live.size(), lacx_digest{});
    std::vector<int> rcs(live.size(), LACX_OK);
    float ms = 0.f;
    const int rc = lacx_decoder_digest_pcm_batch_device(t.d, src.data(), (uint32_t)src.size(), t.d->stream, rcs.data(), dg.data(), &ms);
    t.ms += ms;
    if (rc == LACX_E_DEVICE) return rc;
    for (size_t a = 0; a < live.size(); ++a) {  // (nothing k_edit writes can fail these checks: an internal error otherwise)
        const uint32_t i = t.plan.outs[live[a]].src;
        if (rcs[a] != LACX_OK) t.code[i] = rcs[a], t.err[i] = lacx_decoder_item_error(t.d, (uint32_t)a);
    }
    return LACX_OK;
}

// Phase 2: the outputs that survived as one batch encode, each assembled into its file, and verified where asked for.
int encode_outputs(Transcode& t, const std::vector<size_t>& live, const std::vector<lacx_digest>& dg) {
    const size_t n = live.size();
    std::vector<lacx_batch_item> items(n);
    for (size_t a = 0; a < n; ++a) {
        const EditOut& e = t.plan.outs[live[a]];
        items[a] = lacx_batch_item{t.pcm(live[a]), e.frames, e.sample_rate, e.bit_depth, e.stereo_mode, {0, 0}};
    }
    std::vector<lacx_batch_out> bo(n);
    const int rc = lacx_encode_batch_device(t.enc, items.data(), (uint32_t)n, nullptr, bo.data());
    if (rc != LACX_OK) return decode_fail(rc, lacx_last_error(t.enc));
    for (size_t a = 0; a < n; ++a) {
        const EditOut& e = t.plan.outs[live[a]];
        lacx_config cfg = t.enc->cfg;
        cfg.sample_rate = e.sample_rate;
        cfg.bit_depth = e.bit_depth;
        cfg.stereo_mode = e.stereo_mode;
        uint8_t* buf = nullptr;
        uint64_t size = 0;
        const int ac = lacx_assemble(&cfg, e.channels, 1, &bo[a].payload, &bo[a].payload_size, &bo[a].table, &bo[a].nblocks, &buf, &size);
        if (ac != LACX_OK) {
            t.code[e.src] = ac;
            t.err[e.src] = ac == LACX_E_RUNTIME ? "out of memory or a block of no bytes" : "cannot assemble the output";
            continue;
        }
        t.out[e.src] = lacx_span{buf, size};
        if (t.results) {
            lacx_edit_result& r = t.results[e.src];
            r.frames = e.frames;
            r.lac_bytes = size;
            r.blocks = bo[a].nblocks;
            r.data_crc32 = dg[a].data_crc32;
            r.sample_rate = e.sample_rate;
            r.channels = e.channels;
            r.bit_depth = e.bit_depth;
            r.source_lac_bytes = e.source_lac_bytes;
        }
    }
    if (!(t.flags & LACX_TRANSCODE_VERIFY)) return LACX_OK;
    std::vector<lacx_verify_item> vi;
    std::vector<size_t> who;
    for (size_t a = 0; a < n; ++a) {
        const EditOut& e = t.plan.outs[live[a]];
        if (t.code[e.src] != LACX_OK) continue;
        vi.push_back(lacx_verify_item{t.out[e.src].data, t.out[e.src].size, t.pcm(live[a]), e.frames});
        who.push_back(e.src);
    }
    if (vi.empty()) return LACX_OK;
    std::vector<int> vrc(vi.size(), LACX_OK);
    float ms = 0.f;
    const int vc = lacx_decoder_verify_batch_device(t.d, vi.data(), (uint32_t)vi.size(), t.d->stream, vrc.data(), nullptr, &ms);
    t.ms += ms;
    if (vc == LACX_E_DEVICE) return vc;
    for (size_t a = 0; a < vi.size(); ++a) {
        const uint32_t i = (uint32_t)who[a];
        if (vrc[a] == LACX_OK) {
            if (t.results) t.results[i].verified = 1;
            continue;
        }
        t.code[i] = LACX_E_MISMATCH;
        t.err[i] = std::string("[transcode-error] output does not decode to its sources: ") + lacx_decoder_item_error(t.d, (uint32_t)a);
    }
    return LACX_OK;
}

// The device half.  LACX_OK, or the whole call's failure (its words in lacx_decode_last_error).
int run(Transcode& t) {
    lacx_decoder* d = t.d;
    int prev_device = -1;
    if (DevErr e = decoder_open(d, &prev_device)) return device_fail(e);
    int rc = ensure_device(t.enc);
    if (rc != LACX_OK) rc = decode_fail(rc, lacx_last_error(t.enc));
    else if (t.enc->device != d->device) rc = decode_fail(LACX_E_INVALID, "the encoder is on another device than the decoder");
    if (rc == LACX_OK) {
        DevErr e = chk(hipSetDevice(d->device), "hipSetDevice");
        if (!e) e = buf_grow(d->edit_stage, t.plan.stage_elems, 0);
        if (!e) e = buf_grow(d->edit_dst, t.plan.dst_bytes, 0);
        if (e) rc = device_fail(e);
    }
    if (rc == LACX_OK) rc = decode_segments(t);
    if (rc == LACX_OK) rc = edit_outputs(t);
    std::vector<size_t> live;
    for (size_t j = 0; rc == LACX_OK && j < t.plan.outs.size(); ++j)
        if (t.alive(j)) live.push_back(j);
    std::vector<lacx_digest> dg;
    if (rc == LACX_OK && !live.empty()) rc = digest_outputs(t, live, dg);
    if (rc == LACX_OK) {
        std::vector<size_t> keep;
        std::vector<lacx_digest> kd;
        for (size_t a = 0; a < live.size(); ++a)
            if (t.alive(live[a])) keep.push_back(live[a]), kd.push_back(dg[a]);
        if (!keep.empty()) rc = encode_outputs(t, keep, kd);
    }
    if (prev_device >= 0) (void)hipSetDevice(prev_device);
    return rc;
}

}  // namespace

int lacx_transcode_batch(lacx_decoder* d, lacx_encoder* enc, const lacx_edit_segment* segs, uint32_t nsegs, const lacx_edit_output* outs,
                         uint32_t nouts, uint32_t flags, lacx_span* out, int* item_rc, lacx_edit_result* results, float* device_ms) {
    if (device_ms) *device_ms = 0.f;
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!enc) return decode_fail(LACX_E_INVALID, "null encoder");
    if (!segs || !outs || !out || nouts == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    if (flags & ~LACX_TRANSCODE_VERIFY) return decode_fail(LACX_E_INVALID, "unknown flags");
    if (is_fanout(enc)) return decode_fail(LACX_E_INVALID, "a transcode job needs an encoder on one device, not a fan-out");
    if (enc->cfg.device >= 0 && d->device >= 0 && enc->cfg.device != d->device)
        return decode_fail(LACX_E_INVALID, "the encoder is on another device than the decoder");
    // both handles for the whole call: two jobs that share one of them take turns (std::scoped_lock orders the two locks)
    const std::shared_ptr<std::mutex> dec_mu = d->call_mu;
    std::scoped_lock lock(*dec_mu, enc->call_mu);
    for (uint32_t i = 0; i < nouts; ++i) out[i] = lacx_span{nullptr, 0};
    if (results) std::memset(results, 0, sizeof(lacx_edit_result) * nouts);
    EditPlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    plan_edit(segs, nsegs, outs, nouts, plan, code, err);
    Transcode t{d, enc, segs, flags, plan, code, err, out, results};
    int rc = LACX_OK;
    if (lacx_device_count() <= 0) rc = decode_fail(LACX_E_DEVICE, "no usable HIP device");
    else if (!plan.outs.empty()) rc = run(t);
    if (device_ms) *device_ms = t.ms;
    for (uint32_t i = 0; i < nouts; ++i) {
        if (rc != LACX_OK && code[i] == LACX_OK) code[i] = rc, err[i] = lacx_decode_last_error();  // the whole call failed
        if (code[i] == LACX_OK) continue;
        lacx_free(const_cast<uint8_t*>(out[i].data));
        out[i] = lacx_span{nullptr, 0};
        if (results) results[i] = lacx_edit_result{};
    }
    if (item_rc) std::copy(code.begin(), code.end(), item_rc);
    d->item_err = std::move(err);
    if (rc != LACX_OK) return rc;
    for (uint32_t i = 0; i < nouts; ++i)
        if (code[i] != LACX_OK) return decode_fail(code[i], "output " + std::to_string(i) + ": " + d->item_err[i]);
    return LACX_OK;
}
