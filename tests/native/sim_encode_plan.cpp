// sim_encode_plan.cpp -- prints the encoder's host-only plans (csrc/encode_plan.h) for the commands on its standard
// input, one JSON line per command; tests/test_encode_plan_host.py states the rules independently and compares.  Built
// from encode_plan.h alone (no ROCm include path: the header is host-only), plain and with AddressSanitizer + UBSan.
//
//   chunks nb device_emit fused upload pipe_chunks split
//   shard  frames channels bit_depth stereo_mode layout host_src  fused direct packer persistent lazy halves pinned_cap pipe_chunks split
//   batch  n pinned_cap exact  then per item: frames rate depth mode channels layout data0 data1 exact_cap
//   sizes  nb channels  then nb frame counts, then nb * channels size records
// (split "-": none; data0 / data1: 0 null, 1 set, 3 set and refused by the import check)
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>

#include "encode_plan.h"

using namespace lacx;

static PlanKnobs read_knobs(std::istream& in, bool all) {
    PlanKnobs kn;
    if (all) in >> kn.fused_emit >> kn.direct_packer >> kn.packer >> kn.persistent >> kn.lazy_repair >> kn.front_halves >> kn.pinned_cap_bytes;
    in >> kn.pipe_chunks >> kn.pipe_split;
    if (kn.pipe_split == "-") kn.pipe_split.clear();
    return kn;
}

static void cmd_chunks(std::istream& in) {
    uint32_t nb;
    bool device_emit, fused, upload;
    in >> nb >> device_emit >> fused >> upload;
    const PlanKnobs kn = read_knobs(in, false);
    const std::vector<Chunk> c = plan_chunks(kn, nb, device_emit, fused, upload);
    std::printf("{\"chunks\":[");
    for (size_t i = 0; i < c.size(); ++i) std::printf("%s[%u,%u]", i ? "," : "", c[i].first, c[i].count);
    std::printf("]}\n");
}

static void print_caps(const Capacities& c) {
    std::printf("\"cap\":{\"dev_payload\":%" PRIu64 ",\"pinned_payload\":%" PRIu64 ",\"prefix\":%" PRIu64 ",\"pinned_fresh\":%d,\"ranges\":%u,"
                "\"table_blocks\":%u,\"emitted\":%u,\"sizes\":%u,\"batch_table\":%" PRIu64 "}",
                c.dev_payload, c.pinned_payload, c.prefix, (int)c.pinned_fresh, c.ranges, c.table_blocks, c.emitted, c.sizes, c.batch_table);
}

static void cmd_shard(std::istream& in) {
    ShardIn si;
    in >> si.frames >> si.channels >> si.bit_depth >> si.stereo_mode >> si.layout >> si.host_src;
    const PlanKnobs kn = read_knobs(in, true);
    const ShardPlan p = plan_shard(si, kn);
    std::printf("{\"nb\":%u,\"frame_bytes\":%" PRIu64 ",\"fused\":%d,\"packer\":%d,\"drained\":%d,\"direct\":%d,\"lazy\":%d,\"persistent\":%d,"
                "\"front_halves\":%d,\"fuse_items\":%u,\"ranges\":%u,",
                p.nb, p.frame_bytes, (int)p.fused, (int)p.packer, (int)p.drained, (int)p.direct, (int)p.lazy, (int)p.persistent,
                (int)p.front_halves, p.fuse_items, p.ranges);
    print_caps(p.cap);
    std::printf(",\"chunks\":[");
    for (size_t i = 0; i < p.chunks.size(); ++i) {
        const ChunkPlan& k = p.chunks[i];
        std::printf("%s{\"first\":%u,\"count\":%u,\"f0\":%" PRIu64 ",\"f1\":%" PRIu64 ",\"src_off\":%" PRIu64 ",\"stream_base\":%u,\"fuse_items\":%u,"
                    "\"stream\":%d,\"block_off_at\":%u,\"err_at\":%u,\"t_first_at\":%u,\"t_last_at\":%u,\"work_ctr_at\":%u}",
                    i ? "," : "", k.first, k.count, k.f0, k.f1, k.src_off, k.stream_base, k.fuse_items, k.stream, k.block_off_at, k.err_at,
                    k.t_first_at, k.t_last_at, k.work_ctr_at);
    }
    std::printf("]}\n");
}

static const char* import_stub(const lacx_pcm& p, int) { return (uintptr_t)p.data0 == 3 ? "refused by the import check" : nullptr; }

static void cmd_batch(std::istream& in) {
    uint32_t n;
    PlanKnobs kn;
    bool exact;
    in >> n >> kn.pinned_cap_bytes >> exact;
    std::vector<lacx_batch_item> items(n);
    std::vector<uint64_t> caps(n);
    for (uint32_t i = 0; i < n; ++i) {
        lacx_batch_item& it = items[i];
        it = lacx_batch_item{};
        unsigned rate, depth, mode, channels, layout, d0, d1;
        in >> it.frames >> rate >> depth >> mode >> channels >> layout >> d0 >> d1 >> caps[i];
        it.sample_rate = rate;
        it.bit_depth = depth;
        it.stereo_mode = mode;
        it.pcm.channels = channels;
        it.pcm.layout = layout;
        it.pcm.data0 = reinterpret_cast<const void*>((uintptr_t)d0);
        it.pcm.data1 = reinterpret_cast<const void*>((uintptr_t)d1);
    }
    BatchPlan p;
    std::string why;
    const ParamBase pb{1, 0, 7u};
    const int rc = plan_batch(items.data(), n, pb, kn, exact ? caps.data() : nullptr, import_stub, &p, &why);
    if (rc) {
        std::printf("{\"rc\":%d,\"msg\":\"%s\"}\n", rc, why.c_str());
        return;
    }
    std::printf("{\"rc\":0,\"nb\":%u,\"nitems\":%u,\"max_depth\":%d,\"tab_bytes\":%zu,\"map_bytes\":%zu,\"sizeof_desc\":%zu,", p.nb, p.nitems,
                p.max_depth, p.tab_bytes, p.map_bytes, sizeof(StreamDesc));
    print_caps(p.cap);
    std::printf(",\"streams\":[");
    for (uint32_t i = 0; i < n; ++i) {
        const StreamDesc& s = p.streams[i];
        std::printf("%s{\"frames\":%" PRIu64 ",\"num_blocks\":%u,\"channels\":%d,\"stereo_mode\":%d,\"bit_depth\":%d,\"layout\":%d,\"zero_run\":%d,"
                    "\"partitioning\":%d,\"debug_skip\":%u,\"stream_base\":%u,\"first_block\":%u,\"first_wg\":%u,\"fuse_items\":%u,\"pad\":%u,"
                    "\"out_base\":%llu,\"out_cap\":%llu,\"imported\":%d,\"null_ptrs\":%d}",
                    i ? "," : "", (uint64_t)s.prm.frames, s.prm.num_blocks, s.prm.channels, s.prm.stereo_mode, s.prm.bit_depth, s.prm.layout,
                    s.prm.zero_run, s.prm.partitioning, s.prm.debug_skip, s.prm.stream_base, s.first_block, s.first_wg, s.fuse_items, s.pad,
                    s.out_base, s.out_cap, (int)p.imported[i], (int)(s.left == nullptr && s.right == nullptr));
    }
    std::printf("],\"item_stream\":[");
    for (size_t i = 0; i < p.item_stream.size(); ++i) std::printf("%s%u", i ? "," : "", (unsigned)p.item_stream[i]);
    std::printf("]}\n");
}

static void cmd_sizes(std::istream& in) {
    uint32_t nb;
    int channels;
    in >> nb >> channels;
    std::vector<BlockPlan> bplans(nb);  // (every buffer at exactly the size the encoder provides: the sanitizers watch)
    std::vector<unsigned long long> recs((size_t)nb * channels);
    std::vector<uint32_t> table((size_t)nb * 2);
    for (auto& b : bplans) {
        b = BlockPlan{};
        in >> b.frames;
    }
    for (auto& r : recs) in >> r;
    const SizeTable t = table_from_size_records(recs.data(), bplans.data(), nb, channels, table.data());
    std::printf("{\"total\":%llu,\"complete\":%d,\"table\":[", t.total, (int)t.complete);
    for (size_t i = 0; i < table.size(); ++i) std::printf("%s%u", i ? "," : "", table[i]);
    // the batch's per-stream byte sums over the same table: a stream of the last nb - 1 blocks
    StreamDesc sd{};
    sd.first_block = nb > 1 ? 1 : 0;
    sd.prm.num_blocks = nb > 1 ? nb - 1 : 1;
    bool empty = false;
    const uint64_t bytes = batch_stream_bytes(table.data(), sd, &empty);
    std::printf("],\"tail_bytes\":%" PRIu64 ",\"tail_empty\":%d}\n", bytes, (int)empty);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "chunks") cmd_chunks(in);
        else if (cmd == "shard") cmd_shard(in);
        else if (cmd == "batch") cmd_batch(in);
        else if (cmd == "sizes") cmd_sizes(in);
        else if (!cmd.empty()) return 2;
    }
    return 0;
}
