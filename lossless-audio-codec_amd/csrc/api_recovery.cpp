// api_recovery.cpp -- the recovery data's entry points of the C ABI (lacx.h): the plan is recovery_plan.h's, run here on
// the decoder's device.  The arena lies in the decoder's payload buffer, the tables in its table buffers, what a call
// hands out in its pinned stage buffer.
#include "decode_plan.h"
#include "decoder_impl.h"
#include "encoder_impl.h"
#include "recovery_plan.h"

// (the entry points are declared extern "C" in lacx.h)
namespace {

DevErr run_ups(lacx_decoder* d, const std::vector<RecUp>& ups, hipStream_t st) {
    for (const RecUp& u : ups)
        if (DevErr e = u.src ? chk(hipMemcpyAsync(d->d_pay() + u.at, u.src, u.bytes, hipMemcpyHostToDevice, st), "H2D recovery input")
                             : chk(hipMemsetAsync(d->d_pay() + u.at, 0, u.bytes, st), "memset"))
            return e;
    return DevErr{};
}

// One stage: its tables up, its kernels between the decoder's two events, its CRC words and `downs` down, and the wait.
DevErr run_stage(lacx_decoder* d, const RecStage& stage, const std::vector<RecDown>& downs, uint64_t out_bytes, hipStream_t st, float* device_ms,
                 std::vector<uint32_t>& crc) {
    crc.assign(stage.ranges.size(), 0);
    if (stage.size)
        if (DevErr e = buf_grow(d->tables, stage.size, stage.size / 8 + 256)) return e;
    if (out_bytes)
        if (DevErr e = buf_grow(d->stage, out_bytes, 0)) return e;
    if (!stage.empty()) {
        stage.fill(d->h_meta());
        if (DevErr e = chk(hipMemcpyAsync(d->d_meta(), d->h_meta(), stage.size, hipMemcpyHostToDevice, st), "H2D recovery tables")) return e;
        RecoveryArgs a;
        a.arena = d->d_pay();
        a.tasks = reinterpret_cast<const GfTask*>(d->d_meta() + stage.at_tasks);
        std::copy(stage.tier_t0, stage.tier_t0 + kGfTiers + 1, a.tier_t0);
        std::copy(stage.tier_wgs, stage.tier_wgs + kGfTiers, a.tier_wgs);
        a.refs = reinterpret_cast<const unsigned long long*>(d->d_meta() + stage.at_refs);
        a.mat = d->d_meta() + stage.at_mat;
        a.ranges = reinterpret_cast<const CrcRange*>(d->d_meta() + stage.at_ranges);
        a.nranges = (uint32_t)stage.ranges.size();
        a.crc = reinterpret_cast<uint32_t*>(d->d_meta() + stage.at_crc);
        if (DevErr e = chk(hipEventRecord(d->e0, st), "event record")) return e;
        if (DevErr e = chk(launch_recovery(a, st), "recovery launch")) return e;
        if (DevErr e = chk(hipEventRecord(d->e1, st), "event record")) return e;
        if (a.nranges)
            if (DevErr e = chk(hipMemcpyAsync(d->h_meta() + stage.at_crc, d->d_meta() + stage.at_crc, 4 * (size_t)a.nranges, hipMemcpyDeviceToHost, st),
                               "D2H slice checksums"))
                return e;
    }
    for (const RecDown& x : downs)
        if (DevErr e = chk(hipMemcpyAsync(d->h_pay() + x.out_at, d->d_pay() + x.at, x.bytes, hipMemcpyDeviceToHost, st), "D2H recovery output")) return e;
    if (DevErr e = chk(hipStreamSynchronize(st), "synchronize")) return e;
    if (!stage.empty()) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, d->e0, d->e1);
        if (device_ms) *device_ms += ms;
        if (!crc.empty()) std::memcpy(crc.data(), d->h_meta() + stage.at_crc, 4 * crc.size());
    }
    return DevErr{};
}

// The per-item outcome into item_rc and d->item_err; back the whole call's failure, else the lowest failing item's code
// with "stream i: <message>".
int batch_outcome(lacx_decoder* d, int rc, std::vector<int>& code, std::vector<std::string>& err, int* item_rc, lacx_span* out) {
    if (rc != LACX_OK)
        for (size_t i = 0; i < code.size(); ++i)
            if (code[i] == LACX_OK || code[i] == LACX_E_MISMATCH) code[i] = rc, err[i] = lacx_decode_last_error();
    for (size_t i = 0; out && i < code.size(); ++i)
        if (rc != LACX_OK) out[i] = lacx_span{nullptr, 0};
    if (item_rc) std::copy(code.begin(), code.end(), item_rc);
    d->item_err = std::move(err);
    if (rc != LACX_OK) return rc;
    for (size_t i = 0; i < code.size(); ++i)
        if (code[i] != LACX_OK) return decode_fail(code[i], "stream " + std::to_string(i) + ": " + d->item_err[i]);
    return LACX_OK;
}

int device_failure(const DevErr& e) { return decode_fail(LACX_E_DEVICE, std::string(e.what) + ": " + hipGetErrorString(e.e)); }

// scan (out == null, flags unused) or repair
int scan_or_repair(lacx_decoder* d, const lacx_span* files, const lacx_span* sides, uint32_t n, bool repair, uint32_t flags, lacx_span* out, int* item_rc,
                   lacx_repair_result* results, float* device_ms) {
    if (device_ms) *device_ms = 0.f;
    if (results) std::memset(results, 0, sizeof(lacx_repair_result) * n);
    for (uint32_t i = 0; out && i < n; ++i) out[i] = lacx_span{nullptr, 0};
    d->item_bad.assign(n, {});
    std::vector<int> code;
    std::vector<std::string> err;
    RecRepairPlan plan;
    plan_recovery_scan(files, sides, n, plan, code, err);
    int rc = lacx_device_count() <= 0 ? decode_fail(LACX_E_DEVICE, "no usable HIP device") : LACX_OK;
    if (rc == LACX_OK && plan.scan.ranges.size() >= (1ull << 31)) rc = decode_fail(LACX_E_DEVICE, "batch holds 2^31 slices or more");
    if (rc == LACX_OK && !plan.items.empty()) {
        int prev_device = -1;
        DevErr e = decoder_open(d, &prev_device);
        hipStream_t st = d->stream;
        std::vector<uint32_t> crc;
        if (!e) e = buf_grow(d->pay, plan.arena_bytes, plan.arena_bytes / 8);
        if (!e) e = run_ups(d, plan.ups, st);
        if (!e) e = run_stage(d, plan.scan, {}, 0, st, device_ms, crc);
        if (!e) {
            recovery_classify(plan, crc.data(), !repair, code, err);
            if (repair) {
                plan_recovery_fix(plan, flags, code, err);
                e = run_stage(d, plan.fix, plan.downs, plan.out_bytes, st, device_ms, crc);
                if (!e) recovery_fix_finish(plan, crc.data(), d->h_pay(), out, code, err);
            }
        }
        if (prev_device >= 0) (void)hipSetDevice(prev_device);
        if (e) rc = device_failure(e);
        for (const RecItem& it : plan.items) {
            if (rc != LACX_OK) break;
            d->item_bad[it.src] = it.bad;
            if (results) results[it.src] = it.res;
        }
    }
    if (rc != LACX_OK) {
        d->item_bad.assign(n, {});
        if (results) std::memset(results, 0, sizeof(lacx_repair_result) * n);
    }
    return batch_outcome(d, rc, code, err, item_rc, out);
}

int malloc_copy(const lacx_span& view, uint8_t** out, uint64_t* out_size) {
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(view.size ? view.size : 1));
    if (!buf) return decode_fail(LACX_E_RUNTIME, "out of host memory");
    std::memcpy(buf, view.data, view.size);
    *out = buf;
    *out_size = view.size;
    return LACX_OK;
}

// a batch of one carries no "stream 0: "
int one_outcome(lacx_decoder* d, int rc, int item_code) {
    if (rc == LACX_OK || item_code == LACX_OK || rc != item_code) return rc;
    return decode_fail(item_code, d->item_err.empty() ? std::string() : d->item_err[0]);
}

}  // namespace

int lacx_recovery_parse(const uint8_t* sidecar, uint64_t size, lacx_recovery_info* info) {
    if (info) std::memset(info, 0, sizeof(*info));
    RecGeometry geo;
    std::string why;
    const int rc = recovery_parse(sidecar, size, geo, info, why);
    return rc == LACX_OK ? rc : decode_fail(rc, why);
}

int lacx_recovery_build_batch_view(lacx_decoder* d, const lacx_span* lacs, uint32_t n, const lacx_recovery_params* params, lacx_span* out,
                                   int* item_rc, float* device_ms) {
    if (device_ms) *device_ms = 0.f;
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || !out || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    for (uint32_t i = 0; i < n; ++i) out[i] = lacx_span{nullptr, 0};
    uint32_t S, r, K;
    std::string why;
    if (rec_params(params, S, r, K, why) != LACX_OK) return decode_fail(LACX_E_INVALID, why);
    std::vector<int> code(n, LACX_OK);
    std::vector<std::string> err(n);
    for (uint32_t i = 0; i < n; ++i) {  // a sidecar protects a stream: what the strict parse refuses is refused here
        lacx_stream_info info;
        const char* text = "";
        if ((code[i] = parse_stream(lacs[i].data, lacs[i].size, &info, &text)) != LACX_OK) err[i] = text;
    }
    RecBuildPlan plan;
    plan_recovery_build(lacs, n, S, r, K, plan, code, err);
    int rc = lacx_device_count() <= 0 ? decode_fail(LACX_E_DEVICE, "no usable HIP device") : LACX_OK;
    if (rc == LACX_OK && plan.stage.ranges.size() >= (1ull << 31)) rc = decode_fail(LACX_E_DEVICE, "batch holds 2^31 slices or more");
    if (rc == LACX_OK && !plan.items.empty()) {
        int prev_device = -1;
        DevErr e = decoder_open(d, &prev_device);
        std::vector<uint32_t> crc;
        if (!e) e = buf_grow(d->pay, plan.arena_bytes, plan.arena_bytes / 8);
        if (!e) e = run_ups(d, plan.ups, d->stream);
        if (!e) e = run_stage(d, plan.stage, plan.downs, plan.out_bytes, d->stream, device_ms, crc);
        if (prev_device >= 0) (void)hipSetDevice(prev_device);
        if (e) rc = device_failure(e);
        else recovery_build_finish(plan, crc.data(), d->h_pay(), out);
    }
    return batch_outcome(d, rc, code, err, item_rc, out);
}

int lacx_recovery_build(lacx_decoder* d, const uint8_t* lac, uint64_t size, const lacx_recovery_params* params, uint8_t** out, uint64_t* out_size,
                        float* device_ms) {
    if (out) *out = nullptr;
    if (out_size) *out_size = 0;
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!out || !out_size) return decode_fail(LACX_E_INVALID, "null argument");
    const lacx_span in{lac, size};
    lacx_span view{nullptr, 0};
    int code = LACX_OK;
    const int rc = one_outcome(d, lacx_recovery_build_batch_view(d, &in, 1, params, &view, &code, device_ms), code);
    return rc != LACX_OK ? rc : malloc_copy(view, out, out_size);
}

int lacx_recovery_scan_batch(lacx_decoder* d, const lacx_span* files, const lacx_span* sidecars, uint32_t n, int* item_rc,
                             lacx_repair_result* results, float* device_ms) {
    if (device_ms) *device_ms = 0.f;
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!files || !sidecars || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    return scan_or_repair(d, files, sidecars, n, false, 0, nullptr, item_rc, results, device_ms);
}

int lacx_recovery_repair_batch_view(lacx_decoder* d, const lacx_span* files, const lacx_span* sidecars, uint32_t n, uint32_t flags, lacx_span* out,
                                    int* item_rc, lacx_repair_result* results, float* device_ms) {
    if (device_ms) *device_ms = 0.f;
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!files || !sidecars || !out || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    return scan_or_repair(d, files, sidecars, n, true, flags, out, item_rc, results, device_ms);
}

int lacx_recovery_repair(lacx_decoder* d, const uint8_t* file, uint64_t size, const uint8_t* sidecar, uint64_t sidecar_size, uint32_t flags,
                         uint8_t** out, uint64_t* out_size, lacx_repair_result* result, float* device_ms) {
    if (out) *out = nullptr;
    if (out_size) *out_size = 0;
    if (result) std::memset(result, 0, sizeof(*result));
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!out || !out_size) return decode_fail(LACX_E_INVALID, "null argument");
    const lacx_span in{file, size}, side{sidecar, sidecar_size};
    lacx_span view{nullptr, 0};
    int code = LACX_OK;
    const int rc = one_outcome(d, lacx_recovery_repair_batch_view(d, &in, &side, 1, flags, &view, &code, result, device_ms), code);
    if (!view.data) return rc;
    const int mrc = malloc_copy(view, out, out_size);  // (best effort: an output beside LACX_E_MISMATCH)
    return mrc != LACX_OK ? mrc : rc;
}

int lacx_decoder_item_bad_slices(const lacx_decoder* d, uint32_t i, const uint32_t** slices, uint32_t* count) {
    if (slices) *slices = nullptr;
    if (count) *count = 0;
    if (!d || !slices || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (i >= d->item_bad.size()) return decode_fail(LACX_E_INVALID, "no such item in the last recovery call");
    *slices = d->item_bad[i].data();
    *count = (uint32_t)d->item_bad[i].size();
    return LACX_OK;
}
