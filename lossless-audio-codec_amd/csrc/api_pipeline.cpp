// api_pipeline.cpp -- the launch pipelines: analysis-only, host-emit pipeline (plans D2H, emit workers), device-emit
// pipeline (fused emit, streaming packer, copy-engine drain, repair kernels, regrow), and the many-streams-as-one-job batch.
// Encode calls are pipelined: the stream is cut into chunks of blocks whose kernels alternate between a few HIP streams.
// What the device-emit steps are told comes from the host-only plans of encode_plan.h.
#include "encoder_impl.h"

namespace lacx_host {

// Enqueues the kernels + plan D2H of one chunk on stream `st`, then records done[c].
int enqueue_chunk(lacx_encoder* e, const int32_t* d_left, const int32_t* d_right, uint64_t frames, int channels,
                  int stereo_mode, int bit_depth, const Chunk& ck, int c, hipStream_t st) {
    const uint64_t f0 = (uint64_t)ck.first * kMaxBlock;
    const uint64_t f1 = std::min<uint64_t>(frames, (uint64_t)(ck.first + ck.count) * kMaxBlock);
    const AnalyzeParams prm = make_params(e, f1 - f0, channels, stereo_mode, bit_depth);
    const DeviceWorkspace w = ws_at(e->ws, ck.first);
    LaunchSet ls = one_stream_set(prm, d_left + f0, d_right ? d_right + f0 : nullptr);
    HIP_TRY(e, launch_analysis(bind(ls), w, st, e->ev[c]), "kernel launch");
    HIP_TRY(e, hipMemcpyAsync(e->h_plans + (size_t)ck.first * kSlotsPerBlock, w.plans,
                              (size_t)ck.count * kSlotsPerBlock * sizeof(ChannelPlan), hipMemcpyDeviceToHost, st),
            "D2H plans");
    HIP_TRY(e, hipMemcpyAsync(e->h_bplans + ck.first, w.bplans, (size_t)ck.count * sizeof(BlockPlan),
                              hipMemcpyDeviceToHost, st),
            "D2H block plans");
    HIP_TRY(e, hipEventRecord(e->done[c], st), "event record");
    return LACX_OK;
}

// Runs the kernels on device-resident PCM in one launch set on `st`; leaves plans in the pinned buffers.
int analyze_on_device(lacx_encoder* e, const int32_t* d_left, const int32_t* d_right, uint64_t frames,
                      int channels, int stereo_mode, int bit_depth, hipStream_t st) {
    const uint32_t nb = blocks_for(frames);
    int rc = ensure_workspace(e, nb);
    if (rc) return rc;
    const auto t0 = clk::now();
    const Chunk all{0, nb};
    rc = enqueue_chunk(e, d_left, d_right, frames, channels, stereo_mode, bit_depth, all, 0, st);
    if (rc) return rc;
    HIP_TRY(e, hipEventSynchronize(e->done[0]), "event synchronize");
    e->timing.d2h_ms = ms_since(t0);
    reset_device_timing(e);
    add_chunk_timing(e, 0);
    e->timing.full_launches = 1;
    count_slots(e, 0, nb);
    return LACX_OK;
}

// Pipelined analysis + emit.  `head` bytes are reserved in front of the payload (container header +
// table for whole-stream calls, 0 for shards).  On success *buf_out holds head + payload (malloc'd).
int encode_pipelined(lacx_encoder* e, const int32_t* d_left, const int32_t* d_right, const int32_t* h_left,
                     const int32_t* h_right, uint64_t frames, hipStream_t user_stream, uint64_t head,
                     uint8_t** buf_out, uint64_t* payload_size, std::vector<uint64_t>& offsets) {
    const int channels = d_right ? 2 : 1;
    const uint32_t nb = blocks_for(frames);
    int rc = ensure_workspace(e, nb);
    if (rc) return rc;
    const StreamParams sp = stream_params(e->cfg, channels);
    const std::vector<Chunk> chunks = plan_chunks(e->knobs, nb);
    const uint64_t cap = payload_upper_bound(frames, channels, nb);
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(head + cap));
    if (!buf) return fail(e, LACX_E_RUNTIME, "out of memory");
    offsets.assign((size_t)nb + 1, 0);

    reset_device_timing(e);
    const auto t0 = clk::now();
    // the caller's stream (if any) carries chunks 0, 2, ...; the encoder's second stream the others
    hipStream_t st[kStreams];
    for (int i = 0; i < kStreams; ++i) st[i] = e->stream[i];
    if (user_stream) st[0] = user_stream;
    // Work the caller queued on its stream (e.g. the kernel or copy that produces the PCM) must be ordered before
    // every chunk, also those that run on the encoder's own streams: they wait for an event recorded on st[0].
    {
        const hipError_t pe = hipEventRecord(e->prologue, st[0]);
        if (pe != hipSuccess) {
            std::free(buf);
            return hip_fail(e, pe, "event record");
        }
    }
    for (size_t c = 0; c < chunks.size(); ++c) {
        if (c % kStreams != 0) {
            const hipError_t we = hipStreamWaitEvent(st[c % kStreams], e->prologue, 0);
            if (we != hipSuccess) {
                (void)hipDeviceSynchronize();
                std::free(buf);
                return hip_fail(e, we, "stream wait");
            }
        }
        rc = enqueue_chunk(e, d_left, d_right, frames, channels, e->cfg.stereo_mode, e->cfg.bit_depth, chunks[c],
                           (int)c, st[c % kStreams]);
        if (rc) {
            (void)hipDeviceSynchronize();
            std::free(buf);
            return rc;
        }
    }
    EmitPool& pool = pool_of(e);
    pool.begin(sp, h_left, h_right, frames, e->h_bplans, e->h_plans, nb, offsets.data(), buf + head);
    uint64_t off = 0;
    int status = LACX_OK;
    for (size_t c = 0; c < chunks.size(); ++c) {
        const hipError_t he = hipEventSynchronize(e->done[c]);
        if (he != hipSuccess) {
            status = hip_fail(e, he, "event synchronize");
            break;
        }
        const Chunk& ck = chunks[c];
        bool bad = false;
        for (uint32_t b = ck.first; b < ck.first + ck.count; ++b) {
            if (e->h_bplans[b].invalid) bad = true;
            offsets[b] = off;
            off += block_payload_bytes(sp, e->h_bplans[b], e->h_plans + (size_t)b * kSlotsPerBlock);
        }
        offsets[ck.first + ck.count] = off;
        if (bad || off > cap) {
            status = bad ? LACX_E_INVALID : fail(e, LACX_E_RUNTIME, "payload exceeds the reserved bound");
            break;
        }
        pool.publish(ck.first + ck.count);
    }
    e->timing.d2h_ms = ms_since(t0);
    if (status != LACX_OK) {
        pool.abort();
        (void)pool.finish();
        (void)hipDeviceSynchronize();
        std::free(buf);
        if (status == LACX_E_INVALID) {
            const int rr = check_sample_range(e, nb);  // formats the reference's message
            return rr ? rr : fail(e, LACX_E_INVALID, "sample outside the configured PCM bit depth");
        }
        return status;
    }
    const bool ok = pool.finish();
    for (size_t c = 0; c < chunks.size(); ++c) {
        add_chunk_timing(e, (int)c);
        count_slots(e, chunks[c].first, chunks[c].count);
    }
    e->timing.full_launches = (uint32_t)chunks.size();
    if (!ok) {
        std::free(buf);
        return fail(e, LACX_E_RUNTIME, "emitted size disagrees with the device plan (internal error)");
    }
    uint8_t* shrunk = static_cast<uint8_t*>(std::realloc(buf, (head + off) ? (head + off) : 1));
    *buf_out = shrunk ? shrunk : buf;
    *payload_size = off;
    return LACX_OK;
}

// ---- device-emit pipeline ---------------------------------------------------------------------------------------------
// Per chunk the kernels also produce the bitstream (fused emit + packer, k_offsets + k_pack / k_emit), at global byte
// offsets (chunk c starts where chunk c-1 ends); results stay in encoder-owned pinned memory (e->h_payload, e->h_table()).
// encode_plan.h decides what every step below is told (ShardPlan); the steps only enqueue it.
namespace {

// The address the device uses for a pinned host buffer.
template <class T>
T* mapped(T* host) {
    void* d = nullptr;
    return hipHostGetDevicePointer(&d, host, 0) == hipSuccess ? static_cast<T*>(d) : nullptr;
}

// Where the analysis kernel of a launch set whose per-chunk words are w's leaves its bitstreams.
FuseArgs fuse_args(const lacx_encoder* e, const DeviceWorkspace& w) {
    FuseArgs fa;
    fa.slots = e->ws.slots;
    fa.slot_stride = e->ws.slot_stride;
    fa.emitted = e->ws.emitted;
    fa.err_flag = w.err_flag;
    fa.size_rec = e->ws.size_rec;
    fa.ready_rec = e->ws.ready_rec;
    fa.silent = e->knobs.silent_template ? e->d_silent : nullptr;
    fa.silent_copies = e->ws.err_flag + kMaxChunks + 4;
    return fa;
}

// Kernel arguments of pipeline chunk c of the shard in flight.
struct ChunkCtx {
    AnalyzeParams prm;
    const int32_t* left;
    const int32_t* right;
    DeviceWorkspace w;
    // the chunk as a launch set of one stream; fuse_items: how many of its stream indices take part in the fused emit,
    // out_cap: capacity of the result buffer (offsets are shard-wide: out_base 0)
    LaunchSet set(uint32_t fuse_items, uint64_t out_cap) const { return one_stream_set(prm, left, right, fuse_items, out_cap); }
};
ChunkCtx chunk_ctx(const lacx_encoder* e, size_t c) {
    const ShardPlan& p = e->pend.plan;
    const ChunkPlan& k = p.chunks[c];
    ChunkCtx x;
    x.prm = make_params(e, k.f1 - k.f0, p.in.channels, p.in.stereo_mode, p.in.bit_depth, p.in.layout);
    x.prm.stream_base = k.stream_base;
    auto at = [&](const int32_t* base) { return reinterpret_cast<const int32_t*>(reinterpret_cast<const uint8_t*>(base) + k.src_off); };
    x.left = at(e->pend.d_left);
    x.right = (!p.in.layout && e->pend.d_right) ? at(e->pend.d_right) : nullptr;
    x.w = ws_at(e->ws, k.first);
    x.w.block_off = e->ws.block_off + k.block_off_at;
    x.w.err_flag = e->ws.err_flag + k.err_at;
    x.w.t_first = e->d_tspan + k.t_first_at;
    x.w.t_last = e->d_tspan + k.t_last_at;
    x.w.work_ctr = e->d_work_ctr + k.work_ctr_at;
    return x;
}

// What the host reads after a launch set, in one kernel that stores into the pinned buffers: block rows [first, first +
// count) of the host arrays (w stands at `first`), the packed flags of stream indices [item0, item0 + items), the
// per-chunk words at index c.
enum : unsigned { kGatherBplans = 1, kGatherTable = 2, kGatherTotal = 4, kGatherSizes = 8, kGatherPacker = 16, kGatherTspan = 32 };
struct GatherJob {
    uint32_t first = 0, count = 0, item0 = 0, items = 0;
    size_t c = 0;
    unsigned what = 0;
};
bool gather_list(lacx_encoder* e, const DeviceWorkspace& w, const GatherJob& j, GatherList& g) {
    bool ok = true;
    auto map_if = [&](bool wanted, auto* host) {
        auto* m = wanted ? mapped(host) : nullptr;
        ok = ok && (m || !wanted);
        return m;
    };
    BlockPlan* m_bplans = map_if(j.what & kGatherBplans, e->h_bplans);
    uint32_t* m_table = map_if(j.what & kGatherTable, e->h_table());
    unsigned long long* m_sizes = map_if(j.what & kGatherSizes, e->h_sizes());
    unsigned long long* m_totals = map_if(j.what & (kGatherTotal | kGatherSizes), e->h_totals);
    uint32_t* m_err = map_if(true, e->h_err);
    uint32_t* m_emitted = map_if(j.items != 0, e->h_emitted());
    unsigned long long* m_tspan = map_if(j.what & kGatherTspan, e->h_tspan);
    if (!ok) return false;
    if (m_bplans) g.add(w.bplans, m_bplans + j.first, (size_t)j.count * sizeof(BlockPlan));
    if (m_sizes) {
        g.add(e->ws.size_rec, m_sizes, (size_t)j.items * sizeof(unsigned long long));
        // the "all kernels done" word: any record (its valid bit makes it non-zero); the host puts the total there
        g.add(e->ws.size_rec, &m_totals[j.c], sizeof(unsigned long long));
    }
    if (m_table) g.add(w.table, m_table + (size_t)j.first * 2, (size_t)j.count * 2 * sizeof(uint32_t));
    if (j.what & kGatherTotal) g.add(w.block_off + j.count, &m_totals[j.c], sizeof(unsigned long long));
    g.add(w.err_flag, &m_err[j.c], sizeof(uint32_t));
    // the packer's error flags, moved count, waves that gave up, k_pack's repacked count, the silent copies
    if (j.what & kGatherPacker) g.add(e->ws.err_flag + kMaxChunks, &m_err[kMaxChunks], 5 * sizeof(uint32_t));
    if (m_emitted) g.add(e->ws.packed + j.item0, m_emitted + j.item0, (size_t)j.items * sizeof(uint32_t));
    if (m_tspan) {
        g.add(w.t_first, &m_tspan[j.c], sizeof(unsigned long long));
        g.add(w.t_last, &m_tspan[kMaxChunks + j.c], sizeof(unsigned long long));
    }
    return true;
}

// Statistics of a fused emit over `items` stream indices, from the gathered words.
void fused_emit_stats(lacx_encoder* e, size_t items) {
    e->timing.emit_direct = 0;
    for (size_t i = 0; i < items; ++i) e->timing.emit_direct += e->h_emitted()[i] == 1u;
    e->timing.packer_gave_up = e->h_err[kMaxChunks + 2];
    e->timing.moved_by_k_pack = e->h_err[kMaxChunks + 3];
    e->timing.silent_copies = e->h_err[kMaxChunks + 4];
}
// Device timing of launch set c beyond add_chunk_timing: the emit kernels, and the whole-block kernel's execution span.
void add_emit_timing(lacx_encoder* e, size_t c) {
    float f = 0;
    if (hipEventElapsedTime(&f, e->ev[c][4], e->ev[c][5]) == hipSuccess) e->timing.emit_ms += f;
    (void)hipGetLastError();
    const unsigned long long a = ~e->h_tspan[c], b = e->h_tspan[kMaxChunks + c];  // the start stamp is kept inverted
    if (b > a) e->timing.full_exec_ms += (double)(b - a) * 1e-5;  // 100 MHz device clock -> ms
}

// The pinned result buffer: `prefix` bytes, then `cap` bytes of payload (h_payload_cap is what the kernels are told).
int ensure_pinned(lacx_encoder* e, uint64_t prefix, uint64_t cap, bool fresh, const char* what = nullptr) {
    if (cap > e->h_payload_cap || prefix > e->h_prefix || fresh) {
        buf_free(e->pinned);
        e->h_payload = nullptr;
        e->h_payload_cap = e->h_prefix = 0;
        if (const DevErr d = buf_grow(e->pinned, prefix + cap, 0)) return hip_fail(e, d.e, what ? what : d.what);
        e->h_payload_cap = cap;
        e->h_prefix = prefix;
    }
    e->h_payload = e->pinned.as<uint8_t>() + e->h_prefix;  // (a batch's regions start where the shard path's payload does)
    return LACX_OK;
}
int ensure_capacities(lacx_encoder* e, const Capacities& c) {
    int rc = c.dev_payload ? grow(e, e->dev_payload, c.dev_payload) : LACX_OK;
    if (!rc && c.ranges) rc = grow(e, e->ranges, c.ranges);
    if (!rc) rc = ensure_pinned(e, c.prefix, c.pinned_payload, c.pinned_fresh);
    if (!rc) rc = grow(e, e->table, c.table_blocks);
    if (!rc && c.emitted) rc = grow(e, e->emitted, c.emitted);
    if (!rc && c.sizes) rc = grow(e, e->sizes, c.sizes);
    if (!rc && c.batch_table) rc = grow(e, e->batch, c.batch_table);
    return rc;
}

}  // namespace

// Copy-engine drain of the payload: every range of stream indices the packer has reported complete (a pinned word per
// range) is fetched from the device payload into the pinned result buffer with hipMemcpyAsync on a copy stream of its
// own -- a copy engine, not CUs.  Called from wherever the calling thread waits: the launch phase of an encode whose
// input is still uploading (chunk c's payload leaves while chunk c + 1's PCM arrives: PCIe is full duplex) and the wait
// for the kernels in encode_device_end.
void drain_pump(lacx_encoder* e) {
    if (e->pend.ranges == 0) return;  // (not drained, or the packer is not launched yet)
    const volatile unsigned long long* flags = e->h_range();
    while (e->pend.next_range < e->pend.ranges) {
        const unsigned long long v = flags[e->pend.next_range];
        if (v == 0) break;
        const uint64_t end = v - 1u;
        if (e->knobs.debug_drain)
            std::fprintf(stderr, "[drain] range %u end %llu at %.3f ms\n", e->pend.next_range, (unsigned long long)end, ms_since(e->pend.t0));
        if (end > e->pend.drained_to && end <= e->h_payload_cap) {
            hipStream_t cs = (e->pend.next_range & 1u) && e->knobs.two_copy_streams ? e->copy_stream2 : e->copy_stream;
            if (hipMemcpyAsync(e->h_payload + e->pend.drained_to, e->d_payload() + e->pend.drained_to, end - e->pend.drained_to,
                               hipMemcpyDeviceToHost, cs) != hipSuccess)
                return;  // (the final copy in encode_device_end fetches what is missing)
            e->pend.drained_to = end;
            const double now = ms_since(e->pend.t0);
            if (e->timing.drain_copies == 0) e->timing.drain_first_ms = now;
            e->timing.drain_last_ms = now;
            e->timing.drain_copies += 1;
        }
        ++e->pend.next_range;
    }
}

namespace {

// begin, step 1: the plan, every buffer it needs, and the call's state.
int prepare_shard(lacx_encoder* e, const int32_t* d_left, const int32_t* d_right, uint64_t frames, hipStream_t user_stream,
                  int layout, int layout_channels, bool host_src) {
    ShardIn in;
    in.frames = frames;
    in.channels = layout ? layout_channels : (d_right ? 2 : 1);
    in.bit_depth = e->cfg.bit_depth;
    in.stereo_mode = e->cfg.stereo_mode;
    in.layout = layout;
    in.host_src = host_src;
    auto& pd = e->pend;
    pd.plan = plan_shard(in, e->knobs);
    const ShardPlan& p = pd.plan;
    int rc = ensure_workspace(e, p.nb);
    if (!rc) rc = ensure_capacities(e, p.cap);
    if (!rc && p.fused) rc = ensure_slots(e, p.nb, in.channels);
    if (rc) return rc;
    if (!p.fused) e->ws.slots = nullptr;
    reset_device_timing(e);
    e->timing.emit_ms = 0;
    e->timing.drain_copies = 0;
    e->timing.drain_first_ms = e->timing.drain_last_ms = e->timing.poll_gap_max_ms = e->timing.kernels_done_ms = 0;
    pd.t0 = clk::now();
    pd.ranges = pd.next_range = 0;
    pd.drained_to = 0;
    pd.d_left = d_left;
    pd.d_right = d_right;
    for (int c = 0; c < kMaxChunks; ++c) e->h_totals[c] = 0;  // (the last chunk's total doubles as the "all kernels done" word)
    // the caller's stream (if any) carries chunks 0, 4, ...; the encoder's other streams the others
    for (int i = 0; i < kStreams; ++i) pd.st[i] = e->stream[i];
    if (user_stream) pd.st[0] = user_stream;
    // Destination of the packer and of k_emit: device memory that a copy engine drains, or the pinned host buffer itself
    // (the kernels' 16-byte stores cross PCIe while later blocks are still being analysed).
    pd.emit_dst = e->d_payload();
    pd.emit_cap = std::min<uint64_t>(e->dev_payload.cap, e->h_payload_cap);
    if (p.direct) {
        HIP_TRY(e, hipHostGetDevicePointer((void**)&pd.emit_dst, e->h_payload, 0), "hipHostGetDevicePointer");
        pd.emit_cap = e->h_payload_cap;
    }
    HIP_TRY(e, hipMemsetAsync(e->zero_region, 0, e->zero_bytes, pd.st[0]), "memset");  // records, flags, time stamps, range counters
    // Work the caller queued on its stream must be ordered before every chunk, also those on the encoder's own streams
    HIP_TRY(e, hipEventRecord(e->prologue, pd.st[0]), "event record");
    return LACX_OK;
}

// begin, step 2 (host input): the uploader thread copies the chunks in order and announces each.
int start_upload(lacx_encoder* e, const HostSrc& src) {
    if (!e->uploader) {
        // the thread last: a creation that fails leaves no uploader behind, and the next call makes what is still missing
        if (!e->up_stream) HIP_TRY(e, hipStreamCreateWithFlags(&e->up_stream, hipStreamNonBlocking), "hipStreamCreate");
        for (auto& ev : e->up_ev)
            if (!ev) HIP_TRY(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
        e->uploader.reset(new Worker());
    }
    for (auto& d : e->up_done) d.store(0, std::memory_order_relaxed);
    e->up_ms = 0;
    const std::vector<ChunkPlan> chunks = e->pend.plan.chunks;  // (the thread's own copy)
    const int dev = e->device;
    uint8_t* dst0 = const_cast<uint8_t*>(reinterpret_cast<const uint8_t*>(e->pend.d_left));
    uint8_t* dst1 = const_cast<uint8_t*>(reinterpret_cast<const uint8_t*>(e->pend.d_right));
    e->uploader->post([e, src, chunks, dev, dst0, dst1] {
        (void)hipSetDevice(dev);
        const auto tu0 = clk::now();
        bool ok = true;
        for (size_t c = 0; c < chunks.size(); ++c) {
            const uint64_t o = chunks[c].f0 * src.frame_bytes, nbytes = (chunks[c].f1 - chunks[c].f0) * src.frame_bytes;
            if (ok) ok = hipMemcpyAsync(dst0 + o, src.p0 + o, nbytes, hipMemcpyHostToDevice, e->up_stream) == hipSuccess;
            if (ok && src.p1) ok = hipMemcpyAsync(dst1 + o, src.p1 + o, nbytes, hipMemcpyHostToDevice, e->up_stream) == hipSuccess;
            if (ok) ok = hipEventRecord(e->up_ev[c], e->up_stream) == hipSuccess;
            e->up_done[c].store(ok ? 1 : -1, std::memory_order_release);
        }
        e->up_ms = ms_since(tu0);
    });
    return LACX_OK;
}

// The streaming packer: beside the whole-block analysis kernels, on its own stream.  It starts when the first chunk's
// ingest / Levinson / probe kernels are done (ev[0][2] is recorded right in front of the whole-block kernel), so its
// bounded waits only ever cover the progress of the analysis itself, however long the shard.  (With persistent analysis
// workgroups it has to be resident before they are: it then starts in front of the ingest kernel -- ev[0][0], behind the
// call's memset -- and holds its CUs through the front kernels.)
int launch_packer(lacx_encoder* e, bool persistent) {
    auto& pd = e->pend;
    const ShardPlan& p = pd.plan;
    HIP_TRY(e, hipStreamWaitEvent(e->pack_stream, e->ev[0][persistent ? 0 : 2], 0), "stream wait");
    // (the packer walks the whole shard: one stream whose indices start at 0)
    AnalyzeParams shard_prm = make_params(e, p.in.frames, p.in.channels, p.in.stereo_mode, p.in.bit_depth, p.in.layout);
    shard_prm.stream_base = 0;
    LaunchSet shard = one_stream_set(shard_prm, nullptr, nullptr, p.fuse_items, pd.emit_cap);
    RangeProgress rp;
    if (p.drained) {
        std::memset(e->h_range(), 0, (size_t)p.ranges * sizeof(unsigned long long));
        // (the range counters live in the region the call's one memset clears: a memset on the packer's own stream
        // would make the packer's dispatch wait for everything queued before it, the analysis kernel included)
        rp.range_cnt = e->d_range_cnt;
        rp.range_end = e->d_range_end;
        HIP_TRY(e, hipHostGetDevicePointer((void**)&rp.host_end, e->h_range(), 0), "hipHostGetDevicePointer");
        rp.fuse_total = p.fuse_items;
        rp.fence_mode = e->knobs.drain_fence;
        pd.ranges = p.ranges;  // (from here on drain_pump looks at the flags)
    }
    HIP_TRY(e, launch_stream_out(bind(shard), e->ws, pd.emit_dst, e->ws.err_flag + kMaxChunks, e->pack_stream, rp, e->knobs.tune), "packer launch");
    HIP_TRY(e, hipEventRecord(e->pack_done, e->pack_stream), "event record");
    return LACX_OK;
}

// begin, step 3, chunk c: its front and analysis kernels (and, behind the first chunk's, the packer).
int enqueue_analysis(lacx_encoder* e, size_t c, bool host_src) {
    auto& pd = e->pend;
    const ShardPlan& p = pd.plan;
    hipStream_t s = pd.st[p.chunks[c].stream];
    if (s != pd.st[0]) HIP_TRY(e, hipStreamWaitEvent(s, e->prologue, 0), "stream wait");
    const ChunkCtx cx = chunk_ctx(e, c);
    const FuseArgs fa = p.fused ? fuse_args(e, cx.w) : FuseArgs{};
    if (host_src) {
        // this chunk's PCM is being copied by the uploader thread: wait (on the host) until its copy has been issued and
        // its event recorded, then make the chunk's stream wait for that event
        const auto tw0 = clk::now();
        int st_up = 0;
        while ((st_up = e->up_done[c].load(std::memory_order_acquire)) == 0) {
            drain_pump(e);  // earlier chunks' payload leaves while this chunk's PCM arrives
            __builtin_ia32_pause();
            if (ms_since(tw0) > 20000.0) break;
        }
        if (st_up != 1) return fail(e, LACX_E_DEVICE, "host to device copy of the PCM failed");
        HIP_TRY(e, hipStreamWaitEvent(s, e->up_ev[c], 0), "stream wait");
    }
    LaunchSet ls = cx.set(p.chunks[c].fuse_items, pd.emit_cap);
    DeviceWorkspace wl = cx.w;
    if (!p.persistent) wl.work_ctr = nullptr;
    LaunchTuning tune = e->knobs.tune;
    if (p.front_halves && s != e->stream[kStreams - 1]) {  // (see LaunchTuning::aux_stream)
        tune.aux_stream = e->stream[kStreams - 1];
        tune.aux_ev[0] = e->aux_ev[0];
        tune.aux_ev[1] = e->aux_ev[1];
    }
    // Fused emit: the packer walks the stream indices in order, so the whole-block kernels of the chunks run in that
    // order too (chunk c's waits for chunk c-1's: ev[c-1][3] is recorded behind it); what comes before them --
    // ingest, Levinson, probes -- still overlaps the previous chunk's analysis.
    HIP_TRY(e, launch_analysis(bind(ls), wl, s, e->ev[c], &fa, p.fused && c > 0 ? e->ev[c - 1][3] : nullptr, tune), "kernel launch");
    return c == 0 && p.packer ? launch_packer(e, analysis_is_persistent(wl)) : LACX_OK;
}

// begin, step 4, chunk c: everything behind the analysis.  With the fused emit it waits for the packer (what k_pack /
// k_emit still have to move is only known once the packer has finished), and a stream may carry several chunks, so none
// of this may be enqueued before the last chunk's analysis kernels.
int enqueue_tail(lacx_encoder* e, size_t c) {
    auto& pd = e->pend;
    const ShardPlan& p = pd.plan;
    const ChunkPlan& k = p.chunks[c];
    hipStream_t s = pd.st[k.stream];
    const ChunkCtx cx = chunk_ctx(e, c);
    const uint32_t items = p.nb * (uint32_t)p.in.channels;
    if (p.lazy) {
        // Not even k_offsets: the block table follows from the size records the analysis kernel published (the host
        // adds them up), the repair kernels -- the only readers of the device-side offsets -- are enqueued on demand,
        // k_offsets in front of them.  All that stands between the end of the analysis and the host is the packer's
        // completion and one gather kernel.
        HIP_TRY(e, hipStreamWaitEvent(s, e->pack_done, 0), "stream wait");
    } else {
        // block offsets are global: chunk c starts where chunk c-1 ended (its k_offsets must have run)
        const unsigned long long* prev_end = c ? e->ws.block_off + p.chunks[c - 1].block_off_at + p.chunks[c - 1].count : nullptr;
        LaunchSet ls = cx.set(k.fuse_items, pd.emit_cap);
        HIP_TRY(e, launch_emit(bind(ls), cx.w, pd.emit_dst, prev_end, c ? e->copied[c - 1] : nullptr, e->copied[c], s, true,
                               p.packer ? e->ws.err_flag + kMaxChunks + 1 : nullptr, items, p.packer ? e->pack_done : nullptr,
                               e->ws.err_flag + kMaxChunks + 3, false), "emit launch");
    }
    HIP_TRY(e, hipEventRecord(e->ev[c][5], s), "event record");
    GatherJob j{k.first, k.count, k.stream_base, p.fused ? k.count * (uint32_t)p.in.channels : 0u, c,
                kGatherBplans | kGatherTspan | (p.lazy ? kGatherSizes : kGatherTable | kGatherTotal) |
                    (c + 1 == p.chunks.size() ? kGatherPacker : 0u)};
    GatherList g;
    if (!gather_list(e, cx.w, j, g)) return fail(e, LACX_E_RUNTIME, "hipHostGetDevicePointer failed");
    HIP_TRY(e, launch_gather(g, s), "gather launch");
    HIP_TRY(e, hipEventRecord(e->done[c], s), "event record");
    return LACX_OK;
}

}  // namespace

// Part 1: enqueue everything (no host synchronisation): plan, buffers, upload, per chunk the analysis, the packer, per
// chunk the tail.
int encode_device_begin(lacx_encoder* e, const int32_t* d_left, const int32_t* d_right, uint64_t frames,
                        hipStream_t user_stream, int layout, int layout_channels, const HostSrc* hs) {
    int rc = e->pend.active ? fail(e, LACX_E_RUNTIME, "an encode is already in flight on this encoder") : LACX_OK;
    if (!rc) rc = prepare_shard(e, d_left, d_right, frames, user_stream, layout, layout_channels, hs != nullptr);
    if (!rc && hs) rc = start_upload(e, *hs);
    const size_t chunks = rc ? 0 : e->pend.plan.chunks.size();
    for (size_t c = 0; c < chunks && !rc; ++c) rc = enqueue_analysis(e, c, hs != nullptr);
    for (size_t c = 0; c < chunks && !rc; ++c) rc = enqueue_tail(e, c);
    if (rc == LACX_OK) {
        e->timing.enqueue_ms = ms_since(e->pend.t0);
        e->pend.active = true;
        return rc;
    }
    // A failure half-way leaves kernels queued that write to the workspace, the slots and the pinned result buffer: they
    // must have drained before the next call clears, frees or regrows any of those.
    if (e->uploader) e->uploader->wait();  // (it reads the caller's buffer and writes this encoder's)
    if (e->device_ready) (void)hipDeviceSynchronize();
    return rc;
}

// The pinned result buffer was reserved from an estimate and the stream needs more.  Every chunk's k_offsets has run
// (offsets do not depend on the capacity) and the blocks that did not fit wrote nothing, so the exact total is known:
// regrow the buffer and run only the emit kernels again, chunk by chunk, from the plans still in the workspace.
int reemit_into_regrown_buffer(lacx_encoder* e, uint64_t* payload_size) {
    const size_t chunks = e->pend.plan.chunks.size();
    HIP_TRY(e, hipDeviceSynchronize(), "synchronize");
    const uint64_t total = e->h_totals[chunks - 1];  // cumulative byte count after the last chunk
    const uint64_t cap = total + 4096u;
    const int rc = ensure_pinned(e, e->h_prefix, cap, true, "hipHostMalloc(payload regrow)");  // (the prefix survives)
    if (rc) return rc;
    uint8_t* dst = nullptr;
    HIP_TRY(e, hipHostGetDevicePointer((void**)&dst, e->h_payload, 0), "hipHostGetDevicePointer");
    hipStream_t s = e->stream[0];
    HIP_TRY(e, hipMemsetAsync(e->ws.err_flag, 0, sizeof(uint32_t) * (kMaxChunks + 1), s), "memset");
    const unsigned long long* prev_end = nullptr;
    for (size_t c = 0; c < chunks; ++c) {
        const ChunkCtx cx = chunk_ctx(e, c);
        LaunchSet ls = cx.set(0, cap);
        HIP_TRY(e, launch_emit(bind(ls), cx.w, dst, prev_end, nullptr, nullptr, s, /*skip_emitted=*/false), "emit relaunch");
        prev_end = cx.w.block_off + e->pend.plan.chunks[c].count;
        HIP_TRY(e, hipMemcpyAsync(&e->h_err[c], cx.w.err_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s), "D2H err");
    }
    HIP_TRY(e, hipStreamSynchronize(s), "synchronize");
    for (size_t c = 0; c < chunks; ++c) {
        if (e->h_err[c] & 1u) return fail(e, LACX_E_RUNTIME, "device emit disagrees with the analysis plan (internal error)");
        if ((e->h_err[c] & 2u) || e->h_totals[c] > cap)
            return fail(e, LACX_E_RUNTIME, "payload exceeds the regrown result buffer (internal error)");
    }
    *payload_size = total;
    return LACX_OK;
}

namespace {
constexpr int kTooSmall = -1;  // a step's verdict inside encode_device_end: the reservation was too small (never returned)

// end, step 1: copy-engine drain while the kernels run -- every range of stream indices the packer reports complete is
// fetched from the device payload into the pinned result buffer.
void wait_with_drain(lacx_encoder* e) {
    const size_t last = e->pend.plan.chunks.size() - 1;
    // (no runtime call in the loop but the copies: the gather kernel -- the last one of the call -- stores the
    // cumulative byte count of the last chunk, non-zero, into pinned memory that was zeroed before the launch)
    const volatile unsigned long long* finished = &e->h_totals[last];
    // The loop is a spin on pinned memory with a pause instruction between looks (a sibling hyper-thread keeps its
    // issue slots); every look is time-stamped, so a host thread that was descheduled or busy elsewhere shows up as
    // poll_gap_max_ms instead of as an unexplained long step.  Once a millisecond the last chunk's event is queried as
    // well: a failed device ends the wait even though its completion word never arrives.
    const auto poll0 = clk::now();
    auto last_look = poll0;
    auto last_query = poll0;
    while (*finished == 0ull) {
        drain_pump(e);
        const auto now = clk::now();
        const double gap = std::chrono::duration<double, std::milli>(now - last_look).count();
        if (gap > e->timing.poll_gap_max_ms) e->timing.poll_gap_max_ms = gap;
        last_look = now;
        if (std::chrono::duration<double, std::milli>(now - last_query).count() > 1.0) {
            last_query = now;
            const hipError_t qe = hipEventQuery(e->done[last]);
            if (qe != hipErrorNotReady) break;  // done (the word is about to follow) or failed: the event wait below reports it
            if (std::chrono::duration<double, std::milli>(now - poll0).count() > 20000.0) break;
        }
        __builtin_ia32_pause();
    }
    e->timing.kernels_done_ms = ms_since(e->pend.t0);
    if (e->knobs.debug_drain) std::fprintf(stderr, "[drain] kernels done at %.3f ms, copy stream %s\n", ms_since(e->pend.t0),
                                           hipStreamQuery(e->copy_stream) == hipSuccess ? "idle" : "busy");
    drain_pump(e);
}

// end, step 2 (lazy path): the block table and the payload's size from the size records (k_offsets never ran).
int table_from_records(lacx_encoder* e) {
    const ShardPlan& p = e->pend.plan;
    if (hipEventSynchronize(e->done[0]) != hipSuccess) return LACX_OK;  // (the chunk check reports it)
    const SizeTable t = table_from_size_records(e->h_sizes(), e->h_bplans, p.nb, p.in.channels, e->h_table());
    e->h_totals[0] = t.total;
    bool any_invalid = false;
    for (uint32_t b = 0; b < p.nb; ++b) any_invalid = any_invalid || e->h_bplans[b].invalid;
    if (!t.complete && !any_invalid) return fail(e, LACX_E_RUNTIME, "a channel block's size record is missing (internal error)");
    return LACX_OK;
}

// end, step 3 (lazy path): the packer did not move every channel block -- a wave gave up, a bitstream did not fit its
// slot.  Now the repair kernels run: k_offsets, k_pack for the slots left behind, k_emit for what was never emitted,
// then the gather once more.  (One chunk.  Not a regrow; moved_by_k_pack and packer_gave_up say what happened.)
int enqueue_repair(lacx_encoder* e) {
    const ShardPlan& p = e->pend.plan;
    const uint32_t items = p.nb * (uint32_t)p.in.channels;
    const ChunkCtx cx = chunk_ctx(e, 0);
    LaunchSet ls = cx.set(p.chunks[0].fuse_items, e->pend.emit_cap);
    hipStream_t s = e->pend.st[0];
    hipError_t re = launch_emit(bind(ls), cx.w, e->pend.emit_dst, nullptr, nullptr, nullptr, s, true, e->ws.err_flag + kMaxChunks + 1,
                                items, nullptr, e->ws.err_flag + kMaxChunks + 3, false);
    GatherList g;
    if (re == hipSuccess && gather_list(e, cx.w, GatherJob{0, p.nb, 0, items, 0, kGatherTable | kGatherTotal | kGatherPacker}, g))
        re = launch_gather(g, s);
    if (re == hipSuccess) re = hipEventRecord(e->done[0], s);
    return re == hipSuccess ? LACX_OK : hip_fail(e, re, "repair launch");
}

// end, step 4: wait for the chunks in order and check each; *off: the payload's size so far.
int check_chunks(lacx_encoder* e, uint64_t* off) {
    const ShardPlan& p = e->pend.plan;
    for (size_t c = 0; c < p.chunks.size(); ++c) {
        const hipError_t he = hipEventSynchronize(e->done[c]);
        if (he != hipSuccess) return hip_fail(e, he, "event synchronize");
        const ChunkPlan& k = p.chunks[c];
        for (uint32_t b = k.first; b < k.first + k.count; ++b)
            if (e->h_bplans[b].invalid) return LACX_E_INVALID;
        if (e->h_err[c] & 1u) return fail(e, LACX_E_RUNTIME, "device emit disagrees with the analysis plan (internal error)");
        const uint64_t end = e->h_totals[c];  // cumulative
        const bool packer_overflow = c + 1 == p.chunks.size() && (e->h_err[kMaxChunks] & 2u);
        if ((e->h_err[c] & 2u) || packer_overflow || end > e->h_payload_cap) return kTooSmall;  // re-emit into a regrown buffer
        *off = end;
    }
    return LACX_OK;
}

// end, step 5 (drained): what the ranges did not cover -- the tail, and, when the repair kernels had to place anything
// the packer had counted as done (never seen), everything -- then the copy streams' completion.
int fetch_rest(lacx_encoder* e, int status, uint64_t off) {
    uint64_t drained_to = e->pend.drained_to;
    if (status == LACX_OK) {
        if (e->h_err[kMaxChunks] & 4u) {
            // (range copies of the stale bytes may still be queued on either copy stream: they must have landed before
            // the full copy is enqueued, or one of them could overwrite what k_emit / k_pack placed later)
            (void)hipStreamSynchronize(e->copy_stream2);
            (void)hipStreamSynchronize(e->copy_stream);
            drained_to = 0;
        }
        if (off > drained_to) {
            const hipError_t ce = hipMemcpyAsync(e->h_payload + drained_to, e->d_payload() + drained_to, off - drained_to,
                                                 hipMemcpyDeviceToHost, e->copy_stream);
            if (ce != hipSuccess) status = hip_fail(e, ce, "D2H payload");
        }
    }
    hipError_t se = hipStreamSynchronize(e->copy_stream);
    const hipError_t se2 = hipStreamSynchronize(e->copy_stream2);
    if (se == hipSuccess) se = se2;
    if (se != hipSuccess && status == LACX_OK) status = hip_fail(e, se, "D2H payload");
    return status;
}

// end, step 6: the reservation was too small.  No sample-range error can hide behind the overflow: wait for every
// chunk's block plans first.
int regrow(lacx_encoder* e, uint64_t* off) {
    (void)hipDeviceSynchronize();
    for (uint32_t b = 0; b < e->pend.plan.nb; ++b)
        if (e->h_bplans[b].invalid) return LACX_E_INVALID;
    const int rc = reemit_into_regrown_buffer(e, off);
    e->timing.regrows += 1;
    return rc;
}

// end, step 7: the device's view of the call.
void fill_timing(lacx_encoder* e) {
    const ShardPlan& p = e->pend.plan;
    e->timing.full_exec_ms = 0;
    for (size_t c = 0; c < p.chunks.size(); ++c) {
        add_chunk_timing(e, (int)c);
        add_emit_timing(e, c);
    }
    e->timing.full_launches = (uint32_t)p.chunks.size();
    e->timing.full_slots = (uint64_t)p.nb * (p.in.channels == 2 ? 2u : 1u);
    e->timing.emit_direct = e->timing.moved_by_k_pack = e->timing.packer_gave_up = e->timing.silent_copies = 0;
    if (p.fused) fused_emit_stats(e, (size_t)p.nb * (size_t)p.in.channels);
}

}  // namespace

// Part 2: wait for the kernels (draining the payload meanwhile), build or repair what the lazy path left out, check the
// chunks in order, fetch the rest, regrow if the reservation was too small, hand the result over.
int encode_device_end(lacx_encoder* e, uint64_t* payload_size) {
    if (!e->pend.active) return fail(e, LACX_E_RUNTIME, "no encode in flight on this encoder");
    e->pend.active = false;
    if (e->uploader) {  // (long finished: every chunk's kernels were enqueued behind its copy)
        e->uploader->wait();
        if (e->up_ms > 0) e->timing.h2d_ms = e->up_ms;
        e->up_ms = 0;
    }
    const ShardPlan& p = e->pend.plan;
    if (p.drained) wait_with_drain(e);
    int status = p.lazy ? table_from_records(e) : LACX_OK;
    if (status == LACX_OK && p.lazy && e->h_err[kMaxChunks + 1] != p.nb * (uint32_t)p.in.channels) status = enqueue_repair(e);
    uint64_t off = 0;
    if (const int cs = check_chunks(e, &off)) status = cs;  // (the chunks are waited for whatever came before)
    if (p.drained) status = fetch_rest(e, status, off);
    if (status == kTooSmall) status = regrow(e, &off);
    e->timing.d2h_ms = ms_since(e->pend.t0);
    if (status != LACX_OK) {
        (void)hipDeviceSynchronize();
        if (status == LACX_E_INVALID) {
            const int rr = check_sample_range(e, p.nb);
            return rr ? rr : fail(e, LACX_E_INVALID, "sample outside the configured PCM bit depth");
        }
        return status;
    }
    fill_timing(e);
    *payload_size = off;
    return LACX_OK;
}

int encode_pipelined_device(lacx_encoder* e, const int32_t* d_left, const int32_t* d_right, uint64_t frames,
                            hipStream_t user_stream, uint64_t* payload_size, int layout, int layout_channels,
                            const HostSrc* hs) {
    const int rc = encode_device_begin(e, d_left, d_right, frames, user_stream, layout, layout_channels, hs);
    if (rc) return rc;
    return encode_device_end(e, payload_size);
}

int fetch_pcm_if_needed(lacx_encoder* e, const int32_t* d_left, const int32_t* d_right, uint64_t frames,
                        const int32_t*& h_left, const int32_t*& h_right, std::vector<int32_t>& tl,
                        std::vector<int32_t>& tr) {
    if (h_left) return LACX_OK;
    tl.resize(frames);
    HIP_TRY(e, hipMemcpy(tl.data(), d_left, frames * sizeof(int32_t), hipMemcpyDeviceToHost), "D2H pcm");
    h_left = tl.data();
    if (d_right) {
        tr.resize(frames);
        HIP_TRY(e, hipMemcpy(tr.data(), d_right, frames * sizeof(int32_t), hipMemcpyDeviceToHost), "D2H pcm");
        h_right = tr.data();
    }
    return LACX_OK;
}

// ---- many streams as ONE launch set (lacx_encode_batch_device) ------------------------------------------------------
// Every stream keeps its own parameters (rate, depth, channels, stereo mode, layout); the kernels resolve the stream of a
// block from the descriptor table (StreamDesc, lacx_types.h).  One ingest / Levinson / probe / whole-block launch over
// all blocks of all streams, one packer; every stream's payload lands in its own region of the pinned result buffer.
namespace {

const char* batch_import_error(const lacx_pcm& p, int bit_depth) { return import_source_error(p, bit_depth, true); }

// The job's kernels on s, and the wait for them.
int run_batch(lacx_encoder* e, const LaunchSet& ls, hipStream_t s) {
    const BatchPlan& p = e->batch_plan;
    uint8_t* emit_dst = nullptr;
    HIP_TRY(e, hipHostGetDevicePointer((void**)&emit_dst, e->h_payload, 0), "hipHostGetDevicePointer");
    HIP_TRY(e, hipMemsetAsync(e->zero_region, 0, e->zero_bytes, s), "memset");
    DeviceWorkspace w = e->ws;
    w.t_first = e->d_tspan;
    w.t_last = e->d_tspan + kMaxChunks;
    w.work_ctr = e->knobs.persistent ? e->d_work_ctr : nullptr;
    const FuseArgs fa = fuse_args(e, w);
    HIP_TRY(e, launch_analysis(ls, w, s, e->ev[0], &fa, nullptr, e->knobs.tune), "kernel launch");
    const bool packer = e->knobs.packer;
    if (packer) {
        HIP_TRY(e, hipStreamWaitEvent(e->pack_stream, e->ev[0][analysis_is_persistent(w) ? 0 : 2], 0), "stream wait");
        HIP_TRY(e, launch_stream_out(ls, e->ws, emit_dst, e->ws.err_flag + kMaxChunks, e->pack_stream, RangeProgress{}, e->knobs.tune), "packer launch");
        HIP_TRY(e, hipEventRecord(e->pack_done, e->pack_stream), "event record");
    }
    HIP_TRY(e, launch_emit(ls, w, emit_dst, nullptr, nullptr, nullptr, s, true, packer ? e->ws.err_flag + kMaxChunks + 1 : nullptr,
                           p.nitems, packer ? e->pack_done : nullptr, e->ws.err_flag + kMaxChunks + 3), "emit launch");
    HIP_TRY(e, hipEventRecord(e->ev[0][5], s), "event record");
    GatherList g;
    if (!gather_list(e, w, GatherJob{0, p.nb, 0, p.nitems, 0, kGatherBplans | kGatherTable | kGatherPacker | kGatherTspan}, g))
        return fail(e, LACX_E_RUNTIME, "hipHostGetDevicePointer failed");
    HIP_TRY(e, launch_gather(g, s), "gather launch");
    HIP_TRY(e, hipEventRecord(e->done[0], s), "event record");
    HIP_TRY(e, hipEventSynchronize(e->done[0]), "event synchronize");
    return LACX_OK;
}

// The job as a launch set: the descriptor table and the stream of every stream index are on the device.
LaunchSet batch_set(const lacx_encoder* e) {
    const BatchPlan& p = e->batch_plan;
    LaunchSet ls;
    ls.br.table = reinterpret_cast<const StreamDesc*>(e->d_batch());
    ls.br.nstreams = (uint32_t)p.streams.size();
    ls.br.total_blocks = p.nb;
    ls.br.single = StreamDesc{};
    ls.streams = p.streams.data();
    ls.nstreams = (uint32_t)p.streams.size();
    ls.total_items = p.nitems;
    ls.item_stream = reinterpret_cast<const uint16_t*>(e->d_batch() + p.tab_bytes);
    return ls;
}

// Every stream's result: its region of the pinned buffer and its rows of the block table.
int batch_results(lacx_encoder* e, lacx_batch_out* out) {
    const BatchPlan& p = e->batch_plan;
    for (size_t i = 0; i < p.streams.size(); ++i) {
        const StreamDesc& sd = p.streams[i];
        bool empty = false;
        const uint64_t bytes = batch_stream_bytes(e->h_table(), sd, &empty);
        if (empty) return fail(e, LACX_E_RUNTIME, "encoded block size is outside format limits");
        if (bytes > sd.out_cap) return fail(e, LACX_E_RUNTIME, "a stream's payload exceeds its pinned result reservation");
        out[i].payload = e->h_payload + sd.out_base;
        out[i].payload_size = bytes;
        out[i].table = e->h_table() + 2 * (size_t)sd.first_block;
        out[i].nblocks = sd.prm.num_blocks;
        out[i].reserved = 0;
    }
    return LACX_OK;
}

// Sample-range errors, stream by stream, the reference's wording per stream.
int batch_sample_errors(lacx_encoder* e, const std::vector<int>& imp_item) {
    const BatchPlan& p = e->batch_plan;
    for (uint32_t i = 0; i < p.streams.size(); ++i) {
        const StreamDesc& sd = p.streams[i];
        if (imp_item[i] >= 0)
            if (const int ic = import_check_item(e, (size_t)imp_item[i], true)) return ic;
        for (int pass = 0; pass < 2; ++pass) {
            for (uint32_t b = 0; b < sd.prm.num_blocks; ++b) {
                const BlockPlan& bp = e->h_bplans[sd.first_block + b];
                if (!bp.invalid) continue;
                const bool is_right = (bp.first_bad >> 31) != 0;
                if ((pass == 0) == is_right) continue;
                const uint64_t idx = (uint64_t)b * kMaxBlock + (bp.first_bad & 0x7FFFFFFFu);
                return fail(e, LACX_E_INVALID, "stream " + std::to_string(i) + ": " + (is_right ? "right" : "left") +
                                                   " sample at index " + std::to_string(idx) + " is outside the configured PCM bit depth");
            }
        }
    }
    return LACX_OK;
}

}  // namespace

int encode_batch(lacx_encoder* e, const lacx_batch_item* items, uint32_t n, hipStream_t user_stream, lacx_batch_out* out,
                 const uint64_t* exact_caps) {
    if (e->pend.active) return fail(e, LACX_E_RUNTIME, "an encode is already in flight on this encoder");
    BatchPlan& p = e->batch_plan;
    std::string why;
    if (const int pc = plan_batch(items, n, param_base(e), e->knobs, exact_caps, batch_import_error, &p, &why)) return fail(e, pc, why);
    import_reset(e);
    std::vector<int> imp_item(n, -1);  // streams in a tensor layout: their item of the import pass
    for (uint32_t i = 0; i < n; ++i) {
        int layout = 0;
        if (p.imported[i]) imp_item[i] = import_add(e, items[i].pcm, items[i].frames, items[i].bit_depth, i, &layout);
        p.streams[i].left = static_cast<const int32_t*>(items[i].pcm.data0);
        p.streams[i].right = p.streams[i].prm.layout ? nullptr : static_cast<const int32_t*>(items[i].pcm.data1);
    }
    int rc = ensure_workspace(e, p.nb);
    if (!rc) rc = ensure_slots(e, p.nitems, 1, p.max_depth);  // one stride for the whole set (the deepest material's)
    if (!rc) rc = ensure_capacities(e, p.cap);
    if (rc) return rc;
    reset_device_timing(e);
    e->timing.emit_ms = 0;
    const auto t0 = clk::now();
    hipStream_t s = user_stream ? user_stream : e->stream[0];
    // the streams in a tensor layout: ONE import kernel for all of them, in front of everything else on the job's stream
    rc = import_enqueue(e, s);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i)
        if (imp_item[i] >= 0) p.streams[i].left = import_data(e, imp_item[i]);
    // descriptor table + the stream of every stream index -> device
    HIP_TRY(e, hipMemcpyAsync(e->d_batch(), p.streams.data(), (size_t)n * sizeof(StreamDesc), hipMemcpyHostToDevice, s), "H2D batch table");
    HIP_TRY(e, hipMemcpyAsync(e->d_batch() + p.tab_bytes, p.item_stream.data(), p.map_bytes, hipMemcpyHostToDevice, s), "H2D batch map");
    HIP_TRY(e, hipStreamSynchronize(s), "synchronize");
    rc = run_batch(e, batch_set(e), s);
    if (rc != LACX_OK) (void)hipDeviceSynchronize();
    e->imp.pending = false;  // (looked at below, stream by stream)
    if (rc != LACX_OK) return rc;
    e->timing.d2h_ms = ms_since(t0);
    if (const int sc = batch_sample_errors(e, imp_item)) return sc;
    if (e->h_err[0] & 1u) return fail(e, LACX_E_RUNTIME, "device emit disagrees with the analysis plan (internal error)");
    if ((e->h_err[0] & 2u) || (e->h_err[kMaxChunks] & 2u)) {
        // A stream needs more than its estimated reservation (the single-shard path re-emits into a regrown buffer, the
        // reference never fails on size): k_offsets has run, so the block table holds every stream's exact size -- run the
        // job once more with exact regions.
        if (exact_caps) return fail(e, LACX_E_RUNTIME, "a stream's payload exceeds its exact result reservation (internal error)");
        std::vector<uint64_t> caps(n);
        for (uint32_t i = 0; i < n; ++i) caps[i] = batch_stream_bytes(e->h_table(), p.streams[i]) + 4096u;
        const int rr = encode_batch(e, items, n, user_stream, out, caps.data());
        e->timing.regrows += 1;
        return rr;
    }
    e->timing.full_exec_ms = 0;
    add_chunk_timing(e, 0);
    add_emit_timing(e, 0);
    e->timing.full_launches = 1;
    e->timing.full_slots = p.nitems;
    fused_emit_stats(e, p.nitems);
    if (const int oc = batch_results(e, out)) return oc;
    e->timing.total_ms = ms_since(t0);
    return LACX_OK;
}

}  // namespace lacx_host
