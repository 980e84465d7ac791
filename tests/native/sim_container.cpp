// sim_container.cpp -- drives the .lac container's writer and reader (csrc/container.h) for the commands on its standard
// input, one JSON line per command; tests/test_container_host.py compares with the oracle's streams.  Built from
// container.h alone (no ROCm include path: the header is host-only), plain and with AddressSanitizer + UBSan.
//
//   write rate depth channels mode nb ncuts cut...  then nb rows: frames bytes
//       the head of a stream of those rows, the rows written as ncuts + 1 slices [0, cut0) [cut0, cut1) ... [cut, nb), last
//       slice first; then parse_stream over the head and a payload of the stated sizes, in a buffer of exactly that size
//   offsets nb  then nb frame counts and nb + 1 byte offsets
//       rows_from_offsets
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <vector>

#include "container.h"

using namespace lacx;

static void cmd_write(std::istream& in) {
    StreamParams sp{};
    unsigned depth, channels, mode;
    uint32_t nb, ncuts;
    in >> sp.sample_rate >> depth >> channels >> mode >> nb >> ncuts;
    sp.bit_depth = (uint8_t)depth, sp.channels = (uint8_t)channels, sp.stereo_mode = (uint8_t)mode;
    std::vector<uint32_t> cuts(ncuts), rows(2 * (size_t)nb);
    for (auto& c : cuts) in >> c;
    for (auto& v : rows) in >> v;
    uint64_t pay = 0;
    for (uint32_t b = 0; b < nb; ++b) pay += rows[2 * (size_t)b + 1];
    const uint64_t head = stream_head_bytes(nb), size = head + pay;
    std::unique_ptr<uint8_t[]> lac(new uint8_t[size]);  // exactly the stream: an overrun is the sanitizer's to report
    std::memset(lac.get(), 0xEE, size);
    write_stream_start(sp, nb, lac.get());
    cuts.insert(cuts.begin(), 0u);
    cuts.push_back(nb);
    bool ok = true;
    for (size_t s = cuts.size() - 1; s-- > 0;) ok = write_rows(lac.get(), cuts[s], rows.data() + 2 * (size_t)cuts[s], cuts[s + 1] - cuts[s]) && ok;
    std::printf("{\"ok\":%d,\"head_bytes\":%" PRIu64 ",\"head\":\"", (int)ok, head);
    for (uint64_t i = 0; i < head; ++i) std::printf("%02x", lac[i]);
    lacx_stream_info f{};
    const char* why = "";
    const int rc = parse_stream(lac.get(), size, &f, &why);
    std::printf("\",\"parse\":{\"rc\":%d,\"why\":\"%s\",\"sample_rate\":%u,\"blocks\":%u,\"frames\":%" PRIu64 ",\"channels\":%d,\"bit_depth\":%d,"
                "\"stereo_mode\":%d,\"version\":%d},\"rows\":[",
                rc, rc ? why : "", f.sample_rate, f.blocks, (uint64_t)f.frames, f.channels, f.bit_depth, f.stereo_mode, f.version);
    for (uint32_t b = 0; b < nb; ++b) std::printf("%s%u,%u", b ? "," : "", row_frames(lac.get(), 3, b), row_bytes(lac.get(), b));
    std::printf("]}\n");
}

static void cmd_offsets(std::istream& in) {
    uint32_t nb;
    in >> nb;
    std::vector<BlockPlan> bplans(nb);
    std::vector<uint64_t> offsets((size_t)nb + 1);
    for (auto& bp : bplans) in >> bp.frames;
    for (auto& o : offsets) in >> o;
    std::vector<uint32_t> rows(2 * (size_t)nb, 0);
    const bool ok = rows_from_offsets(offsets.data(), bplans.data(), nb, rows.data());
    std::printf("{\"ok\":%d,\"rows\":[", (int)ok);
    for (size_t i = 0; ok && i < rows.size(); ++i) std::printf("%s%u", i ? "," : "", rows[i]);
    std::printf("]}\n");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "write") cmd_write(in);
        else if (cmd == "offsets") cmd_offsets(in);
        else return std::fprintf(stderr, "unknown command: %s\n", cmd.c_str()), 2;
        if (in.fail()) return std::fprintf(stderr, "short command: %s\n", line.c_str()), 2;
    }
    return 0;
}
