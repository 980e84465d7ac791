// api_import.cpp -- the host side of the import pass (import_core.h, k_import.hip): the checks of a source in a tensor
// layout, the job's item table and destination buffer, the launch in front of the front kernels, and the validation's
// outcome as the reference words it (all of left first, then right: check_sample_range, ref lac/encoder.cpp:82-102).
#include "encoder_impl.h"
#include "import_msg.h"

namespace lacx_host {

const char* import_source_error(const lacx_pcm& p, int bit_depth, bool batch) {
    if (p.layout == LACX_PCM_PLANAR_I16 && bit_depth != 16)
        return batch ? "PCM layout does not match the bit depth" : "PCM layout does not match the configured bit depth";
    const bool planar = p.layout != LACX_PCM_INTERLEAVED_F32;
    if (planar && (p.channels == 2) != (p.data1 != nullptr))
        return "planar PCM: data1 must be the right channel of stereo input and null for mono";
    const uintptr_t mask = p.layout == LACX_PCM_PLANAR_I16 ? 1u : 3u;
    if (((uintptr_t)p.data0 & mask) || (planar && ((uintptr_t)p.data1 & mask)))
        return mask == 1u ? "PCM arrays are not 2-byte aligned" : "PCM arrays are not 4-byte aligned";
    return nullptr;
}

void import_reset(lacx_encoder* e) {
    e->imp.items.clear();
    e->imp.unit_off.assign(1, 0ull);
    e->imp.dst_off.clear();
    e->imp.owner.clear();
    e->imp.bytes = 0;
    e->imp.pending = false;
}

int import_add(lacx_encoder* e, const lacx_pcm& p, uint64_t frames, int bit_depth, uint32_t owner, int* layout) {
    *layout = import_target_layout(bit_depth);
    if (import_is_alias(p.layout, p.channels, p.data0)) return -1;
    ImportItem it{};
    it.src0 = p.data0;
    it.src1 = p.layout == LACX_PCM_INTERLEAVED_F32 ? nullptr : p.data1;
    it.frames = frames;
    it.layout = p.layout;
    it.channels = (uint8_t)p.channels;
    it.bit_depth = (uint8_t)bit_depth;
    e->imp.items.push_back(it);
    e->imp.unit_off.push_back(e->imp.unit_off.back() + (frames + kImportUnitFrames - 1u) / kImportUnitFrames);
    e->imp.dst_off.push_back(e->imp.bytes);
    e->imp.owner.push_back(owner);
    // every item 256-byte aligned, and 16 bytes of look-ahead behind each (the staging loads of the front kernels)
    e->imp.bytes += (frames * p.channels * (uint64_t)(bit_depth / 8) + 16u + 255u) & ~255ull;
    return (int)e->imp.items.size() - 1;
}

int import_enqueue(lacx_encoder* e, hipStream_t s) {
    auto& imp = e->imp;
    const size_t n = imp.items.size();
    if (n == 0) return LACX_OK;
    if (imp.unit_off.back() > 0x7FFFFFFFull) return fail(e, LACX_E_INVALID, "too many frames for one import pass");
    if (const int rc = grow(e, e->import_pcm, imp.bytes)) return rc;
    for (size_t i = 0; i < n; ++i) imp.items[i].dst = e->d_import() + imp.dst_off[i];
    const size_t bad_bytes = (n * sizeof(ImportBad) + 15u) & ~(size_t)15u, item_bytes = (n * sizeof(ImportItem) + 15u) & ~(size_t)15u;
    const size_t tab_bytes = bad_bytes + item_bytes + (n + 1) * sizeof(unsigned long long);
    if (const int rc = grow(e, e->import_tab, tab_bytes)) return rc;
    if (const int rc = grow(e, e->import_bad, n)) return rc;
    ImportBad* bad = reinterpret_cast<ImportBad*>(e->d_import_tab());
    ImportJob job{};
    job.nitems = (uint32_t)n;
    job.total_units = imp.unit_off.back();
    job.single = imp.items[0];
    HIP_TRY(e, hipMemsetAsync(bad, 0xFF, n * sizeof(ImportBad), s), "memset");
    if (n > 1) {  // (the vectors live in the encoder until its next call)
        uint8_t* items = e->d_import_tab() + bad_bytes;
        HIP_TRY(e, hipMemcpyAsync(items, imp.items.data(), n * sizeof(ImportItem), hipMemcpyHostToDevice, s), "H2D import table");
        HIP_TRY(e, hipMemcpyAsync(items + item_bytes, imp.unit_off.data(), (n + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, s),
                "H2D import table");
        job.table = reinterpret_cast<const ImportItem*>(items);
        job.unit_off = reinterpret_cast<const unsigned long long*>(items + item_bytes);
    }
    HIP_TRY(e, launch_import(job, bad, s), "import launch");
    HIP_TRY(e, hipMemcpyAsync(e->h_import_bad(), bad, n * sizeof(ImportBad), hipMemcpyDeviceToHost, s), "D2H import result");
    imp.pending = true;
    return LACX_OK;
}

const int32_t* import_data(const lacx_encoder* e, int item) {
    return reinterpret_cast<const int32_t*>(e->d_import() + e->imp.dst_off[(size_t)item]);
}

int import_check_item(lacx_encoder* e, size_t i, bool batch) {
    int ch = 0;
    unsigned long long idx = 0;
    std::string what;
    if (!import_bad_message(e->h_import_bad()[i], e->imp.items[i].bit_depth, &ch, &idx, what)) return LACX_OK;
    e->bad_channel = ch;
    e->bad_index = idx;
    return fail(e, LACX_E_INVALID, (batch ? "stream " + std::to_string(e->imp.owner[i]) + ": " : std::string()) + what);
}

int import_check(lacx_encoder* e, bool batch) {
    if (!e->imp.pending) return LACX_OK;
    e->imp.pending = false;
    for (size_t i = 0; i < e->imp.items.size(); ++i)  // (in stream order: the items were added that way)
        if (const int rc = import_check_item(e, i, batch)) return rc;
    return LACX_OK;
}

}  // namespace lacx_host
