// lacx_cli -- the `encode`, `decode` and `selftest` commands of the reference's command-line tool on the MI355X path (SURVEY row f-4;
// ref src/main.cpp:609-781).  encode (ref :609-710): same positional arguments, every flag of the reference's encode command with the same
// meaning and rejection rules (--stereo-mode=lr|ms, --no-partitioning, --threads=N, the --debug-* family), LAC_THREADS
// resolved by the tool and not by the library (ref :586-591), the same-file check on the resolved paths (ref :433-444),
// the same messages, staged output (written next to the target, renamed on success).  The WAV file goes through
// lacx_wav_parse / lacx_encode_wav_view: the raw data chunk is what crosses PCIe, the .lac is written to the file
// straight from the encoder's pinned result buffer.  decode (ref :712-781): the same argument checks and messages, the
// .lac parsed on the host first (structural errors need no device), then lacx_decoder_decode_wav_view on the current
// device; the WAV file is written, staged like encode's output, straight from the decoder's pinned image buffer.
// verify (no counterpart in the reference's tool; `flac -t` with the source at hand): a .lac against the WAV it was made
// from, decoded and compared on the device (lacx_decoder_verify_wav) -- no PCM comes back.  encode --verify runs the same
// comparison on the bytes just produced, before the staged output is published (--verify-against=FILE: with another copy
// of the source instead of the input file).  selftest (ref :803-909): the reference's
// four format pairs, signal and frame count, LR / MS / auto / mono encodes through lacx_encode, each verified on the
// device against its source, the header fields read back through lacx_stream_parse, the reference's output lines.
// decode --salvage (no counterpart in the reference's tool; `flac -F`): lacx_decoder_salvage_wav -- whatever blocks of a
// damaged or truncated stream still decode, silence for the others, the lost blocks listed on stderr, exit status 3
// when any was lost.
// digest (no counterpart in the reference's tool; `flac -t` without the source, and the STREAMINFO MD5's role): the CRC-32
// of what every .lac decodes to and of every WAV's data chunk, made on the device (lacx_decoder_digest_batch_device /
// lacx_decoder_digest_pcm_batch_device): a .lac and the WAV it was made from print the same fields.
// stats (no counterpart in the reference's tool; `sox stat` without the floats): the audio statistics of the same two
// kinds of file, made on the device (lacx_decoder_stats_batch_device / lacx_decoder_stats_pcm_batch_device).
// loudness (no counterpart in the reference's tool; `loudgain`, `ffmpeg ebur128`): ITU-R BS.1770 integrated loudness, loudness
// range, momentary and short-term maxima of the same two kinds of file, the K-weighted energy made on the device
// (lacx_decoder_loudness_batch_device / lacx_decoder_loudness_pcm_batch_device).  It only measures.
// peak (the other half of what those tools write): the ITU-R BS.1770 true peak of the same two kinds of file, the 4x
// oversampled maximum made on the device in exact integers (lacx_decoder_truepeak_batch_device /
// lacx_decoder_truepeak_pcm_batch_device).  It only measures.
// spectrum (no counterpart in the reference's tool; `spek`, `sox ... stat -freq`): the long-term power spectrum of the same
// two kinds of file in 64 bands and the bandwidth read off it, the Hann STFT made on the device in FP64
// (lacx_decoder_spectrum_batch_device / lacx_decoder_spectrum_pcm_batch_device).  It only measures.
// accuraterip (what EAC, dBpoweramp, CUETools and whipper print for a rip): the AccurateRip v1 / v2 track checksums of the files
// as one disc of CD audio, made on the device at every read offset within a radius (lacx_decoder_accuraterip_batch_device /
// lacx_decoder_accuraterip_pcm_batch_device).  The database lookup is not part of it.
// compare (what foobar2000's "bit-compare tracks", EAC's "compare WAVs" and `cmp` on decoded audio answer): whether two files
// decode to the same samples, if not how many differ, where and by how much, and whether they do once one is shifted by up to
// 32767 frames, made on the device (lacx_decoder_compare_batch_device / lacx_decoder_compare_pcm_batch_device).
// inspect (`flac -a` for .lac): how each stream was coded and where its bits go, read out of the bytes on the device by a
// parse-only walk (lacx_decoder_inspect_batch_device).
// recompress, cut, join (no counterpart in the reference's tool; `flac -f`, `--skip` / `--until` and joining, for .lac): .lac
// in, .lac out through lacx_transcode_batch -- decoded, edited and encoded again on the device, the PCM never leaving it.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "lacx.h"

namespace {

void usage() {
    std::cerr << "Usage:\n  lacx_cli encode input.wav output.lac [--stereo-mode=lr|ms] [--threads=N] [--debug-threads] [--debug-lpc] "
                 "[--debug-stereo-est] [--debug-zr] [--debug-partitions] [--no-partitioning] [--verify] [--verify-against=other.wav] [--manifest=output.lacm] [--recovery=output.lacr]\n"
                 "  lacx_cli decode input.lac output.wav [--threads=N] [--debug-threads] [--salvage] [--manifest=input.lacm]\n"
                 "      --salvage: decode through errors -- lost blocks become silence, one \"[salvage] block=N ...\" line each on\n"
                 "      stderr; exit 0 when nothing was lost, 3 when the file was written with blocks lost\n"
                 "      --manifest (with --salvage): a block that decodes to something else than its manifest says is lost too\n"
                 "  lacx_cli verify input.lac input.wav\n"
                 "  lacx_cli manifest input.lac output.lacm   (one CRC-32 per block of what the stream decodes to)\n"
                 "  lacx_cli check input.lac input.lacm       (exit 0 intact, 1 damaged: one \"[check] block=N ...\" line each, 2 refused)\n"
                 "  lacx_cli protect input.lac output.lacr [--slice=N] [--parity=R] [--group=K]   (a parity sidecar that brings lost bytes back)\n"
                 "  lacx_cli repair input.lac input.lacr output.lac [--best-effort]\n"
                 "      exit 0 intact or fully repaired, 1 not fully repaired (output.lac only with --best-effort), 2 refused\n"
                 "  lacx_cli digest FILE...   (.lac and .wav files, told apart by content)\n"
                 "  lacx_cli stats FILE... [--blocks]   (.lac and .wav files: peaks, energy, silence and bit use as integers, one line\n"
                 "      per file; --blocks: one further line per block; exit 0 when every file gave statistics, else 1)\n"
                 "  lacx_cli loudness FILE... [--album] [--blocks]   (.lac and .wav files: BS.1770 integrated loudness, range, momentary and\n"
                 "      short-term maxima and gain = -18 - integrated, one line per file; --album: one further line for all files together;\n"
                 "      --blocks: one further line per sub-block of a tenth of a second; nothing is applied to the audio; exit 0 done, 2 refused)\n"
                 "  lacx_cli peak FILE... [--album] [--blocks]   (.lac and .wav files: BS.1770 true peak in dBTP and linear, sample peak in\n"
                 "      dBFS, where the peak lies, `over` for an inter-sample over, one line per file; --album: one further line for all files\n"
                 "      together; --blocks: one further line per 16384 frames; nothing is applied to the audio; exit 0 done, 2 refused)\n"
                 "  lacx_cli spectrum FILE... [--window=N] [--floor=DB] [--blocks]   (.lac and .wav files: per channel the bandwidth -- the upper\n"
                 "      edge of the highest of 64 bands at or above the floor, default -100 dBFS -- and the strongest band, one line per file;\n"
                 "      --window: 256, 512, 1024, 2048 (default) or 4096 frames; --blocks: the 64 levels of every 16384 frames; exit 0 done, 2 refused)\n"
                 "  lacx_cli accuraterip FILE... [--tracks=n0,n1,...] [--radius=N] [--not-first] [--not-last] [--lba0=N] [--match=HEX[,HEX...]]\n"
                 "      (.lac and .wav files of CD audio, together one disc in argument order: the disc ids and per track `NN start frames v1 v2\n"
                 "      s450` at offset 0; --tracks: the track lengths in frames, default one track per file; --radius: read offsets -N .. N,\n"
                 "      at most 2939; --match: every (track, offset, kind) whose sum is one of the values; exit 0 done, 1 nothing matched, 2 refused)\n"
                 "  lacx_cli compare A B [--radius=N] [--centre=N] [--blocks] [--offsets]   (A and B each a .lac or a .wav: the offset of B\n"
                 "      against A with the fewest differing samples among centre - N .. centre + N, N at most 32767, default 0; at it the\n"
                 "      mismatches per channel, the first and last differing time, the peak and RMS of A - B, and the frames only one file has\n"
                 "      at either end; --blocks: one line per 16384 frames; --offsets: the mismatches at every offset searched;\n"
                 "      exit 0 no sample differs at the chosen offset, 1 they differ, 2 refused)\n"
                 "  lacx_cli inspect FILE... [--blocks] [--partitions]   (.lac files: predictors, residual modes and where the bits go, as\n"
                 "      integers, one line per file; --blocks: one further line per block; --partitions: and one per partition;\n"
                 "      a damaged stream prints its line with lost_blocks counted; exit 0 when every file was inspected, else 1)\n"
                 "  lacx_cli recompress in.lac out.lac [--stereo=lr|ms|auto] [--no-zero-run] [--no-partitioning] [--depth=16|24]\n"
                 "      [--channels=keep|left|right|fold|swap|dual] [--verify]   (coded again; depth and channels only where nothing is lost)\n"
                 "  lacx_cli cut in.lac out.lac --start=F [--frames=N] [--verify]   (frames [F, F + N), or to the end)\n"
                 "  lacx_cli join out.lac in1.lac in2.lac ... [--verify]   (streams of one format, one behind the other)\n"
                 "      all three: exit 0 done, 1 mismatch under --verify, 2 refused; out.lac is written only on success\n"
                 "  lacx_cli find FILE... [--quiet=LEVEL|--quiet-db=X] [--peak=LEVEL|--clip] [--flat] [--channel=left|right|all]\n"
                 "      [--min=FRAMES|--min-seconds=S]   (.lac and .wav files: where they are silent, clip or hold one value -- one line\n"
                 "      per run of at least --min frames, then one totals line per detector; exit 0 nothing found, 1 runs found, 2 refused)\n"
                 "  lacx_cli split in.lac PREFIX --quiet=LEVEL --min=FRAMES [--pad=N] [--verify]   (cut at the silences: PREFIX0001.lac ...;\n"
                 "      exit 0 done, 1 mismatch under --verify, 2 refused)\n"
                 "  lacx_cli selftest\n";
}

// A positive decimal integer and nothing else (ref src/main.cpp:560-584, src/codec/lac/thread_limit.hpp:10-28).
bool positive_integer(const std::string& v, unsigned long long& out) {
    if (v.empty() || v.size() > 18) return false;
    for (char c : v)
        if (c < '0' || c > '9') return false;
    out = std::stoull(v);
    return out != 0;
}

// Same target, however the two paths are spelled: an existing file reached twice (hard link, symlink, ./ prefixes), or
// two spellings that normalise to one path when the output does not exist yet (ref src/main.cpp:433-444).
bool same_file(const std::string& a, const std::string& b) {
    std::error_code ec;
    if (std::filesystem::equivalent(a, b, ec)) return true;
    ec.clear();
    const std::filesystem::path na = std::filesystem::weakly_canonical(a, ec);
    if (ec) return false;
    const std::filesystem::path nb = std::filesystem::weakly_canonical(b, ec);
    return !ec && na == nb;
}

// --threads=N when given, else LAC_THREADS (ref src/main.cpp:586-591); false after printing the rejection.  0: neither.
bool resolve_threads(unsigned long long& threads) {
    if (threads == 0) {
        const char* env = std::getenv("LAC_THREADS");
        if (env && *env) {
            const std::string v = env;
            bool digits = true;
            for (char c : v) digits = digits && c >= '0' && c <= '9';
            if (digits && v.size() > 18) {
                std::cerr << "Error: LAC_THREADS is too large\n";
                return false;
            }
            if (!positive_integer(v, threads)) {
                std::cerr << "Error: LAC_THREADS must be a positive integer\n";
                return false;
            }
        }
    }
    return true;
}

// The reference's load_file (ref src/main.cpp:50-63): at most 1 GiB.
bool load_file(const std::string& path, std::vector<uint8_t>& data) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    f.seekg(0, std::ios::end);
    const std::streamsize size = f.tellg();
    if (size < 0 || (unsigned long long)size > (1ull << 30)) return false;
    f.seekg(0, std::ios::beg);
    data.resize((size_t)size);
    if (size > 0) {
        f.read(reinterpret_cast<char*>(data.data()), size);
        if (f.gcount() != size) return false;
    }
    return true;
}

bool save_file(const std::string& path, const uint8_t* data, uint64_t size) {
    const std::string tmp = path + ".lacx-partial";
    bool ok = false;
    {
        std::ofstream out(tmp, std::ios::binary | std::ios::trunc);
        ok = out && out.write(reinterpret_cast<const char*>(data), (std::streamsize)size) && out.flush();
    }
    ok = ok && std::rename(tmp.c_str(), path.c_str()) == 0;
    if (!ok) std::remove(tmp.c_str());
    return ok;
}

// The manifest of what a stream decodes to: its block digests from the device, built on the host.  err: why not.
bool make_manifest(const uint8_t* lac, uint64_t size, std::vector<uint8_t>& out, std::string& err) {
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) return err = "lacx_decoder_create failed", false;
    const lacx_span span{lac, size};
    lacx_digest d{};
    int item_rc = LACX_OK;
    const lacx_block_digest* rows = nullptr;
    uint32_t count = 0;
    uint8_t* m = nullptr;
    uint64_t msize = 0;
    bool ok = false;
    const int rc = lacx_decoder_digest_blocks_batch_device(dec, &span, 1, nullptr, &item_rc, &d, nullptr);
    if (rc != LACX_OK) {
        err = rc == LACX_E_DEVICE ? lacx_decode_last_error() : lacx_decoder_item_error(dec, 0);
    } else if (lacx_decoder_item_block_digests(dec, 0, &rows, &count) != LACX_OK || lacx_manifest_build(&d, rows, count, &m, &msize) != LACX_OK) {
        err = lacx_decode_last_error();
    } else {
        out.assign(m, m + msize);
        lacx_free(m);
        ok = true;
    }
    lacx_decoder_destroy(dec);
    return ok;
}

// lacx_cli manifest input.lac output.lacm
int manifest_command(char** argv) {
    const std::string in_path = argv[2], out_path = argv[3];
    if (same_file(in_path, out_path)) {
        std::cerr << "Input and output paths must be different\n";
        return 1;
    }
    std::vector<uint8_t> lac, m;
    if (!load_file(in_path, lac)) {
        std::cerr << "Failed to read LAC file: " << in_path << "\n";
        return 1;
    }
    std::string err;
    if (!make_manifest(lac.data(), lac.size(), m, err)) {
        std::cerr << "Manifest failed: " << err << "\n";
        return 1;
    }
    if (!save_file(out_path, m.data(), m.size())) {
        std::cerr << "Failed to write manifest: " << out_path << "\n";
        return 1;
    }
    std::cout << "Manifest " << in_path << " -> " << out_path << " (" << (m.size() - 32) / 8 << " blocks)\n";
    return 0;
}

// lacx_cli check input.lac input.lacm: exit 0 when every block decodes to what the manifest says, 1 when the stream is
// damaged or truncated (one line per bad block), 2 when stream or manifest are refused or do not belong together
int check_command(char** argv) {
    const std::string lac_path = argv[2], man_path = argv[3];
    std::vector<uint8_t> lac, man;
    if (!load_file(lac_path, lac)) {
        std::cerr << "Failed to read LAC file: " << lac_path << "\n";
        return 2;
    }
    if (!load_file(man_path, man)) {
        std::cerr << "Failed to read manifest: " << man_path << "\n";
        return 2;
    }
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 2;
    }
    const lacx_span ls{lac.data(), lac.size()}, ms{man.data(), man.size()};
    lacx_salvage_result res{};
    int item_rc = LACX_OK, status = 0;
    const int rc = lacx_decoder_check_batch_device(dec, &ls, &ms, 1, nullptr, &item_rc, &res, nullptr);
    if (rc == LACX_E_MISMATCH && res.blocks) {  // damaged: the device looked at it
        const lacx_block_fault* f = nullptr;
        uint32_t nf = 0;
        if (lacx_decoder_item_faults(dec, 0, &f, &nf) == LACX_OK)
            for (uint32_t k = 0; k < nf; ++k)
                std::cerr << "[check] block=" << f[k].block << " frames=" << f[k].frame << ".." << f[k].frame + f[k].frames - 1 << " "
                          << lacx_block_fault_text(f[k].code) << "\n";
        std::cerr << "Check failed: " << lacx_decoder_item_error(dec, 0) << "\n";
        status = 1;
    } else if (rc != LACX_OK) {
        std::cerr << "Check refused: " << (rc == LACX_E_DEVICE ? lacx_decode_last_error() : lacx_decoder_item_error(dec, 0)) << "\n";
        status = 2;
    } else {
        std::cout << "Intact: " << lac_path << " (" << res.blocks << " blocks, " << res.frames << " samples per channel)\n";
    }
    lacx_decoder_destroy(dec);
    return status;
}

// The recovery sidecar of a file's bytes, made on the device.  err: why not.
bool make_recovery(const uint8_t* lac, uint64_t size, const lacx_recovery_params& prm, std::vector<uint8_t>& out, std::string& err) {
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) return err = "lacx_decoder_create failed", false;
    uint8_t* m = nullptr;
    uint64_t msize = 0;
    const bool ok = lacx_recovery_build(dec, lac, size, &prm, &m, &msize, nullptr) == LACX_OK;
    if (ok) {
        out.assign(m, m + msize);
        lacx_free(m);
    } else {
        err = lacx_decode_last_error();
    }
    lacx_decoder_destroy(dec);
    return ok;
}

// lacx_cli protect input.lac output.lacr [--slice=N] [--parity=R] [--group=K]: exit 0, or 2 where anything is refused
int protect_command(int argc, char** argv) {
    const std::string in_path = argv[2], out_path = argv[3];
    if (same_file(in_path, out_path)) {
        std::cerr << "Input and output paths must be different\n";
        return 2;
    }
    lacx_recovery_params prm{};
    for (int i = 4; i < argc; ++i) {
        const std::string flag = argv[i];
        const std::string sprefix = "--slice=", pprefix = "--parity=", gprefix = "--group=";
        unsigned long long v = 0;
        if (flag.compare(0, sprefix.size(), sprefix) == 0 && positive_integer(flag.substr(sprefix.size()), v) && v <= 0xFFFFFFFFull) {
            prm.slice_bytes = (uint32_t)v;
        } else if (flag.compare(0, pprefix.size(), pprefix) == 0 && positive_integer(flag.substr(pprefix.size()), v) && v <= 0xFFFFull) {
            prm.parity = (uint16_t)v;
        } else if (flag.compare(0, gprefix.size(), gprefix) == 0 && positive_integer(flag.substr(gprefix.size()), v) && v <= 0xFFFFull) {
            prm.group_data = (uint16_t)v;
        } else {
            usage();
            return 2;
        }
    }
    std::vector<uint8_t> lac, m;
    if (!load_file(in_path, lac)) {
        std::cerr << "Failed to read LAC file: " << in_path << "\n";
        return 2;
    }
    std::string err;
    if (!make_recovery(lac.data(), lac.size(), prm, m, err)) {
        std::cerr << "Protect failed: " << err << "\n";
        return 2;
    }
    if (!save_file(out_path, m.data(), m.size())) {
        std::cerr << "Failed to write recovery data: " << out_path << "\n";
        return 2;
    }
    lacx_recovery_info info{};
    (void)lacx_recovery_parse(m.data(), m.size(), &info);
    std::cout << "Protected " << in_path << " -> " << out_path << " (" << m.size() << " bytes: " << info.slices << " slices of " << info.slice_bytes
              << " bytes in " << info.groups << " groups, " << info.parity << " parity slices each)\n";
    return 0;
}

// lacx_cli repair input.lac input.lacr output.lac [--best-effort]: exit 0 when the file is intact or fully repaired, 1
// when it is not (output.lac is written only with --best-effort), 2 when the sidecar is refused or nothing could run
int repair_command(int argc, char** argv) {
    const std::string in_path = argv[2], side_path = argv[3], out_path = argv[4];
    bool best_effort = false;
    for (int i = 5; i < argc; ++i) {
        if (std::string(argv[i]) != "--best-effort") {
            usage();
            return 2;
        }
        best_effort = true;
    }
    if (same_file(in_path, out_path) || same_file(side_path, out_path)) {
        std::cerr << "Input and output paths must be different\n";
        return 2;
    }
    std::vector<uint8_t> file, side;
    if (!load_file(in_path, file)) {
        std::cerr << "Failed to read LAC file: " << in_path << "\n";
        return 2;
    }
    if (!load_file(side_path, side)) {
        std::cerr << "Failed to read recovery data: " << side_path << "\n";
        return 2;
    }
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 2;
    }
    uint8_t* out = nullptr;
    uint64_t out_size = 0;
    lacx_repair_result res{};
    const int rc = lacx_recovery_repair(dec, file.data(), file.size(), side.data(), side.size(), best_effort ? LACX_REPAIR_BEST_EFFORT : 0u, &out, &out_size,
                                        &res, nullptr);
    int status = rc == LACX_OK ? 0 : rc == LACX_E_MISMATCH ? 1 : 2;
    if (status == 2) std::cerr << "Repair refused: " << lacx_decode_last_error() << "\n";
    if (status == 1) std::cerr << "Repair failed: " << lacx_decode_last_error() << "\n";
    if (out && !save_file(out_path, out, out_size)) {
        std::cerr << "Failed to write LAC file: " << out_path << "\n";
        status = 2;
    }
    if (status != 2) {
        const char* flags = (res.flags & LACX_REPAIR_TRUNCATED) ? ", file was cut short" : (res.flags & LACX_REPAIR_TRAILING) ? ", trailing bytes ignored" : "";
        if (status == 0 && res.bad_slices == 0 && !(res.flags & LACX_REPAIR_TRUNCATED))
            std::cout << "Intact: " << in_path << " (" << res.slices << " slices, " << res.parity_slices - res.bad_parity << " of " << res.parity_slices
                      << " parity slices usable" << flags << ")\n";
        else
            std::cout << (status == 0 ? "Repaired: " : "Not repaired: ") << res.repaired_slices << " of " << res.bad_slices << " damaged slices of "
                      << res.slices << " rebuilt, " << res.parity_slices - res.bad_parity << " of " << res.parity_slices << " parity slices usable" << flags
                      << (out ? " -> " + out_path : std::string()) << "\n";
    }
    if (out) lacx_free(out);
    lacx_decoder_destroy(dec);
    return status;
}

constexpr int kExitSalvagedWithLoss = 3;  // decode --salvage: the WAV was written, with lost blocks as silence

// lacx_cli decode input.lac output.wav [--threads=N] [--debug-threads] [--salvage] (ref src/main.cpp:712-781)
int decode_command(int argc, char** argv) {
    const std::string in_path = argv[2], out_path = argv[3];
    if (same_file(in_path, out_path)) {
        std::cerr << "Input and output paths must be different\n";
        return 1;
    }
    bool debug_threads = false, salvage = false;
    unsigned long long threads = 0;
    std::string manifest_path;
    for (int i = 4; i < argc; ++i) {
        const std::string flag = argv[i];
        const std::string tprefix = "--threads=", mprefix = "--manifest=";
        if (flag == "--debug-threads") {
            debug_threads = true;
        } else if (flag == "--salvage") {
            salvage = true;
        } else if (flag.compare(0, mprefix.size(), mprefix) == 0 && flag.size() > mprefix.size()) {
            manifest_path = flag.substr(mprefix.size());
        } else if (flag.compare(0, tprefix.size(), tprefix) == 0) {
            if (!positive_integer(flag.substr(tprefix.size()), threads)) {
                std::cerr << "Error: --threads requires a positive integer\n";
                return 1;
            }
        } else {
            usage();
            return 1;
        }
    }
    if (!resolve_threads(threads)) return 1;  // validated like encode's; the decode itself runs on the device
    if (!manifest_path.empty() && !salvage) {
        std::cerr << "Error: --manifest belongs to --salvage (lacx_cli check answers for the strict decode)\n";
        return 1;
    }
    std::vector<uint8_t> lac, man;
    if (!manifest_path.empty() && !load_file(manifest_path, man)) {
        std::cerr << "Failed to read manifest: " << manifest_path << "\n";
        return 1;
    }
    if (!load_file(in_path, lac)) {
        std::cerr << "Failed to read LAC file: " << in_path << "\n";
        return 1;
    }
    lacx_stream_info info{};
    uint32_t present = 0, scan_flags = 0;
    if ((salvage ? lacx_stream_scan(lac.data(), lac.size(), &info, &present, &scan_flags)
                 : lacx_stream_parse(lac.data(), lac.size(), &info)) != LACX_OK) {  // structural errors need no device
        std::cerr << "Decode failed: " << lacx_decode_last_error() << "\n";
        return 1;
    }
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 1;
    }
    const uint8_t* wav = nullptr;
    uint64_t wav_size = 0;
    lacx_span lac_span{lac.data(), lac.size()}, image{nullptr, 0};
    lacx_salvage_result loss{};
    std::vector<lacx_block_fault> faults;
    if (salvage) {  // a batch of one, as a view: the file is written straight from the pinned image buffer
        int item_rc = LACX_OK;
        const lacx_span man_span{man.data(), man.size()};
        const int rc = manifest_path.empty() ? lacx_decoder_salvage_wav_batch_view(dec, &lac_span, 1, &image, &item_rc, &loss, nullptr)
                                             : lacx_decoder_salvage_wav_batch_view_checked(dec, &lac_span, &man_span, 1, &image, &item_rc, &loss, nullptr);
        if (rc != LACX_OK) {
            std::cerr << "Decode failed: " << (rc == LACX_E_DEVICE ? lacx_decode_last_error() : lacx_decoder_item_error(dec, 0)) << "\n";
            lacx_decoder_destroy(dec);
            return 1;
        }
        const lacx_block_fault* f = nullptr;
        uint32_t nf = 0;
        if (lacx_decoder_item_faults(dec, 0, &f, &nf) == LACX_OK) faults.assign(f, f + nf);
        wav = image.data, wav_size = image.size;
    } else if (lacx_decoder_decode_wav_view(dec, lac.data(), lac.size(), &wav, &wav_size, nullptr) != LACX_OK) {
        std::cerr << "Decode failed: " << lacx_decode_last_error() << "\n";
        lacx_decoder_destroy(dec);
        return 1;
    }
    const std::string tmp = out_path + ".lacx-partial";
    bool ok = false;
    {
        std::ofstream out(tmp, std::ios::binary | std::ios::trunc);
        ok = out && out.write(reinterpret_cast<const char*>(wav), (std::streamsize)wav_size) && out.flush();
    }
    ok = ok && !same_file(in_path, out_path) && std::rename(tmp.c_str(), out_path.c_str()) == 0;
    lacx_decoder_destroy(dec);  // the view dies with the decoder
    if (!ok) {
        std::remove(tmp.c_str());
        std::cerr << "Failed to write WAV: " << out_path << "\n";
        return 1;
    }
    std::cout << "Decoded " << in_path << " -> " << out_path << " (" << info.frames << " samples per channel)\n";
    if (salvage) {
        for (const lacx_block_fault& f : faults)
            std::cerr << "[salvage] block=" << f.block << " frames=" << f.frame << ".." << f.frame + f.frames - 1 << " "
                      << lacx_block_fault_text(f.code) << "\n";
        std::cerr << "[salvage] lost " << loss.bad_blocks << " of " << loss.blocks << " blocks, " << loss.lost_frames << " of "
                  << loss.frames << " frames" << ((loss.flags & LACX_SALVAGE_TRUNCATED) ? ", file truncated" : "")
                  << ((loss.flags & LACX_SALVAGE_TRAILING) ? ", trailing bytes ignored" : "") << "\n";
    }
    if (debug_threads) {
        // The blocks are decoded on the device; on the host the call uses the calling thread, which is what the
        // reference reports for a one-thread run (ref :790-799).
        std::cout << "Decoder thread usage: 1 threads\n  " << std::this_thread::get_id() << "\n";
        std::cout << "WARNING: Decoder multi-threading may not be active.\n";
    }
    return salvage && loss.bad_blocks ? kExitSalvagedWithLoss : 0;
}

// lacx_cli verify input.lac input.wav: exit 0 when the stream decodes to exactly the WAV's samples in the WAV's format
int verify_command(char** argv) {
    const std::string lac_path = argv[2], wav_path = argv[3];
    std::vector<uint8_t> lac, wav;
    if (!load_file(lac_path, lac)) {
        std::cerr << "Failed to read LAC file: " << lac_path << "\n";
        return 1;
    }
    lacx_wav_info winfo{};
    if (!load_file(wav_path, wav) || lacx_wav_parse(wav.data(), wav.size(), &winfo) != LACX_OK) {
        std::cerr << "Failed to read WAV: " << wav_path << "\n";
        return 1;
    }
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 1;
    }
    lacx_verify_result res{};
    const int rc = lacx_decoder_verify_wav(dec, lac.data(), lac.size(), wav.data(), wav.size(), &res, nullptr);
    lacx_decoder_destroy(dec);
    if (rc != LACX_OK) {
        std::cerr << (rc == LACX_E_MISMATCH ? "Verify failed: " : "Decode failed: ") << lacx_decode_last_error() << "\n";
        return 1;
    }
    std::cout << "Verified " << lac_path << " == " << wav_path << " (" << winfo.frames << " samples per channel)\n";
    return 0;
}

// lacx_cli digest FILE...: one line per file that gave a digest, in argument order; the streams are one device job, the
// WAV files' data chunks, uploaded as they are, another.  Exit 0 when every file gave a digest; otherwise the failed
// files' messages on stderr and exit 1.
int digest_command(int argc, char** argv) {
    const int n = argc - 2;
    std::vector<std::vector<uint8_t>> data(n);
    std::vector<std::string> error(n);
    std::vector<lacx_digest> digest(n, lacx_digest{});
    std::vector<int> lacs, wavs;  // indices of the files of each kind that go to the device
    std::vector<lacx_wav_info> winfo(n, lacx_wav_info{});
    for (int i = 0; i < n; ++i) {
        if (!load_file(argv[2 + i], data[i])) {
            error[i] = "Failed to read file";
        } else if (data[i].size() >= 4 && std::memcmp(data[i].data(), "RIFF", 4) == 0) {
            if (lacx_wav_parse(data[i].data(), data[i].size(), &winfo[i]) != LACX_OK) error[i] = "Failed to read WAV";
            else wavs.push_back(i);
        } else {
            lacs.push_back(i);
        }
    }
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 1;
    }
    // the outcome of a batch call for its files: the items' digests and messages
    auto collect = [&](const std::vector<int>& which, int rc, const std::vector<int>& item_rc, const std::vector<lacx_digest>& out) {
        for (size_t k = 0; k < which.size(); ++k) {
            if (item_rc[k] == LACX_OK) digest[which[k]] = out[k];
            else error[which[k]] = rc == LACX_E_DEVICE ? lacx_decode_last_error() : lacx_decoder_item_error(dec, (uint32_t)k);
        }
    };
    if (!lacs.empty()) {
        std::vector<lacx_span> spans;
        for (int i : lacs) spans.push_back(lacx_span{data[i].data(), data[i].size()});
        std::vector<int> item_rc(lacs.size(), LACX_OK);
        std::vector<lacx_digest> out(lacs.size());
        const int rc = lacx_decoder_digest_batch_device(dec, spans.data(), (uint32_t)spans.size(), nullptr, item_rc.data(), out.data(), nullptr);
        collect(lacs, rc, item_rc, out);
    }
    if (!wavs.empty()) {
        std::vector<lacx_digest_source> src;
        std::vector<void*> dev;
        std::vector<int> sent;
        for (int i : wavs) {
            const lacx_wav_info& w = winfo[i];
            const uint64_t bytes = w.frames * w.channels * (uint64_t)(w.bit_depth / 8);
            void* p = nullptr;
            if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess ||
                hipMemcpy(p, data[i].data() + w.data_offset, bytes, hipMemcpyHostToDevice) != hipSuccess) {
                error[i] = "Failed to upload WAV data to the device";
                if (p) (void)hipFree(p);
                continue;
            }
            lacx_digest_source s{};
            s.pcm = lacx_pcm{p, nullptr, w.bit_depth == 16 ? LACX_PCM_INTERLEAVED_I16 : LACX_PCM_INTERLEAVED_I24, w.channels};
            s.frames = w.frames;
            s.sample_rate = w.sample_rate;
            s.bit_depth = (uint8_t)w.bit_depth;
            src.push_back(s), dev.push_back(p), sent.push_back(i);
        }
        if (!src.empty()) {
            std::vector<int> item_rc(src.size(), LACX_OK);
            std::vector<lacx_digest> out(src.size());
            const int rc = lacx_decoder_digest_pcm_batch_device(dec, src.data(), (uint32_t)src.size(), nullptr, item_rc.data(), out.data(), nullptr);
            collect(sent, rc, item_rc, out);
        }
        for (void* p : dev) (void)hipFree(p);
    }
    lacx_decoder_destroy(dec);
    int status = 0;
    for (int i = 0; i < n; ++i) {
        if (!error[i].empty()) {
            std::cerr << "Digest failed: " << argv[2 + i] << ": " << error[i] << "\n";
            status = 1;
            continue;
        }
        const lacx_digest& g = digest[i];
        char line[160];
        std::snprintf(line, sizeof(line), "data_crc32=%08x wav_crc32=%08x frames=%llu channels=%u bits=%u rate=%u ", g.data_crc32, g.wav_crc32,
                      (unsigned long long)g.frames, (unsigned)g.channels, (unsigned)g.bit_depth, (unsigned)g.sample_rate);
        std::cout << line << argv[2 + i] << "\n";
    }
    return status;
}

// a 128-bit value as decimal text (hi: the upper word; negative: two's complement over both words)
std::string dec128(uint64_t lo, uint64_t hi, bool is_signed) {
    const bool neg = is_signed && (hi >> 63) != 0;
    if (neg) {
        lo = ~lo + 1u;
        hi = ~hi + (lo == 0 ? 1u : 0u);
    }
    std::string s;
    do {  // long division by 10, 32 bits at a time
        uint32_t w[4] = {(uint32_t)(hi >> 32), (uint32_t)hi, (uint32_t)(lo >> 32), (uint32_t)lo};
        uint64_t rem = 0;
        for (uint32_t& x : w) {
            const uint64_t cur = (rem << 32) | x;
            x = (uint32_t)(cur / 10u);
            rem = cur % 10u;
        }
        hi = ((uint64_t)w[0] << 32) | w[1], lo = ((uint64_t)w[2] << 32) | w[3];
        s.insert(s.begin(), (char)('0' + rem));
    } while (hi || lo);
    return neg ? "-" + s : s;
}

// lacx_cli stats FILE... [--blocks]: the audio statistics of what every .lac decodes to and of every WAV's data chunk, made on
// the device (lacx_decoder_stats_batch_device / lacx_decoder_stats_pcm_batch_device on the default grid of 16384 frames,
// the encoder's, so that a .lac and the WAV it was made from print the same fields).  One line per file that gave
// statistics, integers only, in argument order; with --blocks one further line per block.  The streams are one device
// job, the WAV files' data chunks, uploaded as they are, another.  Lenient like salvage: a damaged stream prints its line
// with lost_blocks counted.  Exit 0 when every file gave statistics; otherwise the failed files' messages on stderr and
// exit 1.
int stats_command(int argc, char** argv) {
    bool per_block = false;
    std::vector<const char*> paths;
    for (int i = 2; i < argc; ++i) {
        if (std::strcmp(argv[i], "--blocks") == 0) per_block = true;
        else paths.push_back(argv[i]);
    }
    const int n = (int)paths.size();
    if (n == 0) {
        usage();
        return 1;
    }
    std::vector<std::vector<uint8_t>> data(n);
    std::vector<std::string> error(n);
    std::vector<lacx_stats> stats(n, lacx_stats{});
    std::vector<std::vector<lacx_block_stats>> rows(n);
    std::vector<int> lacs, wavs;  // indices of the files of each kind that go to the device
    std::vector<lacx_wav_info> winfo(n, lacx_wav_info{});
    for (int i = 0; i < n; ++i) {
        if (!load_file(paths[i], data[i])) {
            error[i] = "Failed to read file";
        } else if (data[i].size() >= 4 && std::memcmp(data[i].data(), "RIFF", 4) == 0) {
            if (lacx_wav_parse(data[i].data(), data[i].size(), &winfo[i]) != LACX_OK) error[i] = "Failed to read WAV";
            else wavs.push_back(i);
        } else {
            lacs.push_back(i);
        }
    }
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 1;
    }
    // the outcome of a batch call for its files: the items' totals, rows and messages
    auto collect = [&](const std::vector<int>& which, int rc, const std::vector<int>& item_rc, const std::vector<lacx_stats>& out) {
        for (size_t k = 0; k < which.size(); ++k) {
            const lacx_block_stats* r = nullptr;
            uint32_t count = 0;
            if (item_rc[k] == LACX_OK && lacx_decoder_item_block_stats(dec, (uint32_t)k, &r, &count) == LACX_OK) {
                stats[which[k]] = out[k];
                rows[which[k]].assign(r, r + count);
            } else {
                error[which[k]] = rc == LACX_E_DEVICE || item_rc[k] == LACX_OK ? lacx_decode_last_error() : lacx_decoder_item_error(dec, (uint32_t)k);
            }
        }
    };
    if (!lacs.empty()) {
        std::vector<lacx_span> spans;
        for (int i : lacs) spans.push_back(lacx_span{data[i].data(), data[i].size()});
        std::vector<int> item_rc(lacs.size(), LACX_OK);
        std::vector<lacx_stats> out(lacs.size());
        const int rc = lacx_decoder_stats_batch_device(dec, spans.data(), (uint32_t)spans.size(), nullptr, item_rc.data(), out.data(), nullptr);
        collect(lacs, rc, item_rc, out);
    }
    if (!wavs.empty()) {
        std::vector<lacx_digest_source> src;
        std::vector<void*> dev;
        std::vector<int> sent;
        for (int i : wavs) {
            const lacx_wav_info& w = winfo[i];
            const uint64_t bytes = w.frames * w.channels * (uint64_t)(w.bit_depth / 8);
            void* p = nullptr;
            if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess ||
                hipMemcpy(p, data[i].data() + w.data_offset, bytes, hipMemcpyHostToDevice) != hipSuccess) {
                error[i] = "Failed to upload WAV data to the device";
                if (p) (void)hipFree(p);
                continue;
            }
            lacx_digest_source s{};
            s.pcm = lacx_pcm{p, nullptr, w.bit_depth == 16 ? LACX_PCM_INTERLEAVED_I16 : LACX_PCM_INTERLEAVED_I24, w.channels};
            s.frames = w.frames;
            s.sample_rate = w.sample_rate;
            s.bit_depth = (uint8_t)w.bit_depth;
            src.push_back(s), dev.push_back(p), sent.push_back(i);
        }
        if (!src.empty()) {
            std::vector<int> item_rc(src.size(), LACX_OK);
            std::vector<lacx_stats> out(src.size());
            const int rc = lacx_decoder_stats_pcm_batch_device(dec, src.data(), (uint32_t)src.size(), 0, nullptr, item_rc.data(), out.data(), nullptr);
            collect(sent, rc, item_rc, out);
        }
        for (void* p : dev) (void)hipFree(p);
    }
    lacx_decoder_destroy(dec);
    int status = 0;
    for (int i = 0; i < n; ++i) {
        if (!error[i].empty()) {
            std::cerr << "Stats failed: " << paths[i] << ": " << error[i] << "\n";
            status = 1;
            continue;
        }
        const lacx_stats& t = stats[i];
        uint32_t all = 0;
        for (uint32_t c = 0; c < t.channels; ++c) all |= t.ch[c].or_bits;
        uint32_t wasted = t.bit_depth;  // trailing zero bits of the OR over all channels; the whole depth for silence
        if (all) for (wasted = 0; !((all >> wasted) & 1u); ++wasted) {}
        std::cout << "frames=" << t.frames << " channels=" << (unsigned)t.channels << " bits=" << (unsigned)t.bit_depth << " rate=" << t.sample_rate
                  << " blocks=" << t.blocks << " lost_blocks=" << t.lost_blocks << " lead_zero=" << t.lead_zero_frames
                  << " trail_zero=" << t.trail_zero_frames << " silent_blocks=" << t.silent_blocks << " differing=" << t.differing
                  << " wasted_bits=" << wasted;
        for (uint32_t c = 0; c < t.channels; ++c) {
            const lacx_channel_totals& s = t.ch[c];
            std::cout << " ch" << c << ": min=" << s.min << " max=" << s.max << " full_scale=" << s.full_scale << " zeros=" << s.zeros
                      << " sum=" << dec128(s.sum_lo, (uint64_t)s.sum_hi, true) << " sum_sq=" << dec128(s.sum_sq_lo, s.sum_sq_hi, false);
        }
        std::cout << " " << paths[i] << "\n";
        for (size_t b = 0; per_block && b < rows[i].size(); ++b) {
            const lacx_block_stats& r = rows[i][b];
            std::cout << "  block=" << b << " frames=" << r.frames << " code=" << r.code << " lead_zero=" << r.lead_zero_frames
                      << " trail_zero=" << r.trail_zero_frames << " differing=" << r.differing;
            for (uint32_t c = 0; c < t.channels; ++c) {
                const lacx_channel_stats& s = r.ch[c];
                std::cout << " ch" << c << ": min=" << s.min << " max=" << s.max << " or_bits=" << s.or_bits << " full_scale=" << s.full_scale
                          << " zeros=" << s.zeros << " sum=" << (long long)s.sum << " sum_sq=" << (unsigned long long)s.sum_sq;
            }
            std::cout << "\n";
        }
    }
    return status;
}

// lacx_cli loudness FILE... [--album] [--blocks]: the loudness after ITU-R BS.1770 / EBU R 128 of what every .lac decodes to
// and of every WAV's data chunk (lacx_decoder_loudness_batch_device / lacx_decoder_loudness_pcm_batch_device): a .lac and
// the WAV it was made from print the same numbers.  One line per file in argument order: integrated LUFS, range LU,
// momentary and short-term maxima, and gain = -18 - integrated (the ReplayGain 2 reference) -- as text only: nothing is
// ever applied to the audio, gain is not lossless.  --album: one further line for all files together
// (lacx_loudness_combine over every file's rows); --blocks: one further line per sub-block.  The streams are one device
// job, strict like digest; the WAV files' data chunks, uploaded as they are, another.  Exit 0 when every file was measured;
// otherwise the failed files' messages on stderr, nothing on stdout, and exit 2.
std::string loudness_text(const lacx_loudness& t) {
    auto num = [](double x) {
        if (std::isinf(x)) return std::string(x < 0 ? "-inf" : "inf");
        char s[32];
        std::snprintf(s, sizeof(s), "%.2f", x);
        return std::string(s);
    };
    return "integrated=" + num(t.integrated_lufs) + " LUFS range=" + num(t.range_lu) + " LU momentary_max=" + num(t.momentary_max_lufs) +
           " LUFS shortterm_max=" + num(t.shortterm_max_lufs) + " LUFS gain=" + num(-18.0 - t.integrated_lufs) + " dB";
}

int loudness_command(int argc, char** argv) {
    bool album = false, per_block = false;
    std::vector<const char*> paths;
    for (int i = 2; i < argc; ++i) {
        if (std::strcmp(argv[i], "--album") == 0) album = true;
        else if (std::strcmp(argv[i], "--blocks") == 0) per_block = true;
        else paths.push_back(argv[i]);
    }
    const int n = (int)paths.size();
    if (n == 0) {
        usage();
        return 2;
    }
    std::vector<std::vector<uint8_t>> data(n);
    std::vector<std::string> error(n);
    std::vector<lacx_loudness> loud(n, lacx_loudness{});
    std::vector<std::vector<lacx_loudness_row>> rows(n);
    std::vector<int> lacs, wavs;  // indices of the files of each kind that go to the device
    std::vector<lacx_wav_info> winfo(n, lacx_wav_info{});
    for (int i = 0; i < n; ++i) {
        if (!load_file(paths[i], data[i])) {
            error[i] = "Failed to read file";
        } else if (data[i].size() >= 4 && std::memcmp(data[i].data(), "RIFF", 4) == 0) {
            if (lacx_wav_parse(data[i].data(), data[i].size(), &winfo[i]) != LACX_OK) error[i] = "Failed to read WAV";
            else wavs.push_back(i);
        } else {
            lacs.push_back(i);
        }
    }
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 2;
    }
    auto collect = [&](const std::vector<int>& which, int rc, const std::vector<int>& item_rc, const std::vector<lacx_loudness>& out) {
        for (size_t k = 0; k < which.size(); ++k) {
            const lacx_loudness_row* r = nullptr;
            uint32_t count = 0;
            if (item_rc[k] == LACX_OK && lacx_decoder_item_loudness_rows(dec, (uint32_t)k, &r, &count) == LACX_OK) {
                loud[which[k]] = out[k];
                rows[which[k]].assign(r, r + count);
            } else {
                error[which[k]] = rc == LACX_E_DEVICE || item_rc[k] == LACX_OK ? lacx_decode_last_error() : lacx_decoder_item_error(dec, (uint32_t)k);
            }
        }
    };
    if (!lacs.empty()) {
        std::vector<lacx_span> spans;
        for (int i : lacs) spans.push_back(lacx_span{data[i].data(), data[i].size()});
        std::vector<int> item_rc(lacs.size(), LACX_OK);
        std::vector<lacx_loudness> out(lacs.size());
        const int rc = lacx_decoder_loudness_batch_device(dec, spans.data(), (uint32_t)spans.size(), nullptr, item_rc.data(), out.data(), nullptr);
        collect(lacs, rc, item_rc, out);
    }
    if (!wavs.empty()) {
        std::vector<lacx_digest_source> src;
        std::vector<void*> dev;
        std::vector<int> sent;
        for (int i : wavs) {
            const lacx_wav_info& w = winfo[i];
            const uint64_t bytes = w.frames * w.channels * (uint64_t)(w.bit_depth / 8);
            void* p = nullptr;
            if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess ||
                hipMemcpy(p, data[i].data() + w.data_offset, bytes, hipMemcpyHostToDevice) != hipSuccess) {
                error[i] = "Failed to upload WAV data to the device";
                if (p) (void)hipFree(p);
                continue;
            }
            lacx_digest_source s{};
            s.pcm = lacx_pcm{p, nullptr, w.bit_depth == 16 ? LACX_PCM_INTERLEAVED_I16 : LACX_PCM_INTERLEAVED_I24, w.channels};
            s.frames = w.frames;
            s.sample_rate = w.sample_rate;
            s.bit_depth = (uint8_t)w.bit_depth;
            src.push_back(s), dev.push_back(p), sent.push_back(i);
        }
        if (!src.empty()) {
            std::vector<int> item_rc(src.size(), LACX_OK);
            std::vector<lacx_loudness> out(src.size());
            const int rc = lacx_decoder_loudness_pcm_batch_device(dec, src.data(), (uint32_t)src.size(), nullptr, item_rc.data(), out.data(), nullptr);
            collect(sent, rc, item_rc, out);
        }
        for (void* p : dev) (void)hipFree(p);
    }
    lacx_decoder_destroy(dec);
    bool refused = false;
    for (int i = 0; i < n; ++i) {
        if (error[i].empty()) continue;
        std::cerr << "Loudness failed: " << paths[i] << ": " << error[i] << "\n";
        refused = true;
    }
    if (refused) return 2;
    for (int i = 0; i < n; ++i) {
        std::cout << loudness_text(loud[i]) << " " << paths[i] << "\n";
        for (size_t s = 0; per_block && s < rows[i].size(); ++s) {
            char line[128];
            std::snprintf(line, sizeof(line), "  subblock=%zu energy0=%.17g energy1=%.17g", s, rows[i][s].energy[0], rows[i][s].energy[1]);
            std::cout << line << "\n";
        }
    }
    if (album) {
        std::vector<const lacx_loudness_row*> sets;
        std::vector<uint32_t> counts, rates;
        std::vector<uint8_t> channels, depths;
        for (int i = 0; i < n; ++i) {
            sets.push_back(rows[i].data()), counts.push_back((uint32_t)rows[i].size()), rates.push_back(loud[i].sample_rate);
            channels.push_back(loud[i].channels), depths.push_back(loud[i].bit_depth);
        }
        lacx_loudness all{};
        if (lacx_loudness_combine(sets.data(), counts.data(), channels.data(), depths.data(), rates.data(), (uint32_t)n, &all) != LACX_OK) {
            std::cerr << "Loudness failed: album: " << lacx_decode_last_error() << "\n";
            return 2;
        }
        std::cout << loudness_text(all) << " album\n";
    }
    return 0;
}

// lacx_cli peak FILE... [--album] [--blocks]: the true peak after ITU-R BS.1770-4 Annex 2 of what every .lac decodes to and
// of every WAV's data chunk (lacx_decoder_truepeak_batch_device / lacx_decoder_truepeak_pcm_batch_device): a .lac and the WAV
// it was made from print the same numbers.  One line per file in argument order: the true peak in dBTP and as the linear
// value a REPLAYGAIN_*_PEAK tag holds, the sample peak in dBFS, the peak's channel, frame, phase and time, and `over` for an
// inter-sample over.  --album: one further line for all files together (lacx_truepeak_combine over every file's rows; its
// position is the one inside the file named by set=); --blocks: one further line per row of 16384 frames.  Jobs, exit codes
// and messages as `loudness` has them.
std::string peak_text(const lacx_truepeak& t) {
    auto db = [](double x) {
        if (std::isinf(x)) return std::string(x < 0 ? "-inf" : "inf");
        char s[32];
        std::snprintf(s, sizeof(s), "%.2f", x);
        return std::string(s);
    };
    const lacx_truepeak_channel& c = t.ch[t.peak_channel];
    char s[256];
    std::snprintf(s, sizeof(s), " peak=%.6f sample_peak=%s dBFS channel=%u frame=%llu phase=%u time=%.6f", t.true_peak, db(t.sample_peak_dbfs).c_str(),
                  (unsigned)t.peak_channel, (unsigned long long)(c.position / 4u), (unsigned)(c.position % 4u),
                  t.sample_rate ? (double)c.position / (4.0 * t.sample_rate) : 0.0);
    return "true_peak=" + db(t.true_peak_dbtp) + " dBTP" + s + (t.flags & LACX_TRUEPEAK_OVER ? " over" : "");
}

int peak_command(int argc, char** argv) {
    bool album = false, per_block = false;
    std::vector<const char*> paths;
    for (int i = 2; i < argc; ++i) {
        if (std::strcmp(argv[i], "--album") == 0) album = true;
        else if (std::strcmp(argv[i], "--blocks") == 0) per_block = true;
        else paths.push_back(argv[i]);
    }
    const int n = (int)paths.size();
    if (n == 0) {
        usage();
        return 2;
    }
    std::vector<std::vector<uint8_t>> data(n);
    std::vector<std::string> error(n);
    std::vector<lacx_truepeak> peak(n, lacx_truepeak{});
    std::vector<std::vector<lacx_truepeak_row>> rows(n);
    std::vector<int> lacs, wavs;  // indices of the files of each kind that go to the device
    std::vector<lacx_wav_info> winfo(n, lacx_wav_info{});
    for (int i = 0; i < n; ++i) {
        if (!load_file(paths[i], data[i])) {
            error[i] = "Failed to read file";
        } else if (data[i].size() >= 4 && std::memcmp(data[i].data(), "RIFF", 4) == 0) {
            if (lacx_wav_parse(data[i].data(), data[i].size(), &winfo[i]) != LACX_OK) error[i] = "Failed to read WAV";
            else wavs.push_back(i);
        } else {
            lacs.push_back(i);
        }
    }
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 2;
    }
    auto collect = [&](const std::vector<int>& which, int rc, const std::vector<int>& item_rc, const std::vector<lacx_truepeak>& out) {
        for (size_t k = 0; k < which.size(); ++k) {
            const lacx_truepeak_row* r = nullptr;
            uint32_t count = 0;
            if (item_rc[k] == LACX_OK && lacx_decoder_item_truepeak_rows(dec, (uint32_t)k, &r, &count) == LACX_OK) {
                peak[which[k]] = out[k];
                rows[which[k]].assign(r, r + count);
            } else {
                error[which[k]] = rc == LACX_E_DEVICE || item_rc[k] == LACX_OK ? lacx_decode_last_error() : lacx_decoder_item_error(dec, (uint32_t)k);
            }
        }
    };
    if (!lacs.empty()) {
        std::vector<lacx_span> spans;
        for (int i : lacs) spans.push_back(lacx_span{data[i].data(), data[i].size()});
        std::vector<int> item_rc(lacs.size(), LACX_OK);
        std::vector<lacx_truepeak> out(lacs.size());
        const int rc = lacx_decoder_truepeak_batch_device(dec, spans.data(), (uint32_t)spans.size(), nullptr, item_rc.data(), out.data(), nullptr);
        collect(lacs, rc, item_rc, out);
    }
    if (!wavs.empty()) {
        std::vector<lacx_digest_source> src;
        std::vector<void*> dev;
        std::vector<int> sent;
        for (int i : wavs) {
            const lacx_wav_info& w = winfo[i];
            const uint64_t bytes = w.frames * w.channels * (uint64_t)(w.bit_depth / 8);
            void* p = nullptr;
            if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess ||
                hipMemcpy(p, data[i].data() + w.data_offset, bytes, hipMemcpyHostToDevice) != hipSuccess) {
                error[i] = "Failed to upload WAV data to the device";
                if (p) (void)hipFree(p);
                continue;
            }
            lacx_digest_source s{};
            s.pcm = lacx_pcm{p, nullptr, w.bit_depth == 16 ? LACX_PCM_INTERLEAVED_I16 : LACX_PCM_INTERLEAVED_I24, w.channels};
            s.frames = w.frames;
            s.sample_rate = w.sample_rate;
            s.bit_depth = (uint8_t)w.bit_depth;
            src.push_back(s), dev.push_back(p), sent.push_back(i);
        }
        if (!src.empty()) {
            std::vector<int> item_rc(src.size(), LACX_OK);
            std::vector<lacx_truepeak> out(src.size());
            const int rc = lacx_decoder_truepeak_pcm_batch_device(dec, src.data(), (uint32_t)src.size(), nullptr, item_rc.data(), out.data(), nullptr);
            collect(sent, rc, item_rc, out);
        }
        for (void* p : dev) (void)hipFree(p);
    }
    lacx_decoder_destroy(dec);
    bool refused = false;
    for (int i = 0; i < n; ++i) {
        if (error[i].empty()) continue;
        std::cerr << "Peak failed: " << paths[i] << ": " << error[i] << "\n";
        refused = true;
    }
    if (refused) return 2;
    for (int i = 0; i < n; ++i) {
        std::cout << peak_text(peak[i]) << " " << paths[i] << "\n";
        for (size_t s = 0; per_block && s < rows[i].size(); ++s) {
            const lacx_truepeak_row& r = rows[i][s];
            char line[192];
            std::snprintf(line, sizeof(line), "  row=%zu peak0=%llu pos0=%u sample_peak0=%u peak1=%llu pos1=%u sample_peak1=%u", s, (unsigned long long)r.peak[0],
                          r.pos[0], r.sample_peak[0], (unsigned long long)r.peak[1], r.pos[1], r.sample_peak[1]);
            std::cout << line << "\n";
        }
    }
    if (album) {
        std::vector<const lacx_truepeak_row*> sets;
        std::vector<uint32_t> counts, rates;
        std::vector<uint64_t> frames;
        std::vector<uint8_t> channels, depths;
        for (int i = 0; i < n; ++i) {
            sets.push_back(rows[i].data()), counts.push_back((uint32_t)rows[i].size()), rates.push_back(peak[i].sample_rate);
            channels.push_back(peak[i].channels), depths.push_back(peak[i].bit_depth), frames.push_back(peak[i].frames);
        }
        lacx_truepeak all{};
        if (lacx_truepeak_combine(sets.data(), counts.data(), channels.data(), depths.data(), frames.data(), rates.data(), (uint32_t)n, &all) != LACX_OK) {
            std::cerr << "Peak failed: album: " << lacx_decode_last_error() << "\n";
            return 2;
        }
        std::cout << peak_text(all) << " set=" << all.set << " album\n";
    }
    return 0;
}

// lacx_cli spectrum FILE... [--window=N] [--floor=DB] [--blocks]: the banded long-term power spectrum of what every .lac
// decodes to and of every WAV's data chunk (lacx_decoder_spectrum_batch_device / lacx_decoder_spectrum_pcm_batch_device): a
// .lac and the WAV it was made from print the same numbers.  One line per file in argument order: per channel the bandwidth
// (the upper edge of the highest band at or above the floor) and the centre of the strongest band, then the format.
// --blocks: per row of 16384 frames and channel one further line with the 64 band powers (%.17g: every bit).  Jobs, exit
// codes and messages as `peak` has them.
std::string spectrum_text(const lacx_spectrum& t) {
    std::string out;
    for (unsigned c = 0; c < t.channels; ++c) {
        char s[128];
        std::snprintf(s, sizeof(s), "%sch%u: bandwidth=%.1f Hz peak=%.1f Hz", c ? " " : "", c, t.bandwidth_hz[c], (t.peak_band[c] + 0.5) * t.sample_rate / 128.0);
        out += s;
    }
    char s[160];
    std::snprintf(s, sizeof(s), " %u Hz %u bit window=%u windows=%llu floor=%.1f dBFS", t.sample_rate, (unsigned)t.bit_depth, t.window, (unsigned long long)t.windows,
                  t.floor_db);
    return out + s;
}

int spectrum_command(int argc, char** argv) {
    bool per_block = false;
    uint32_t window = 2048;
    double floor_db = -100.0;
    std::vector<const char*> paths;
    for (int i = 2; i < argc; ++i) {
        if (std::strcmp(argv[i], "--blocks") == 0) per_block = true;
        else if (std::strncmp(argv[i], "--window=", 9) == 0) window = (uint32_t)std::strtoul(argv[i] + 9, nullptr, 10);
        else if (std::strncmp(argv[i], "--floor=", 8) == 0) floor_db = std::strtod(argv[i] + 8, nullptr);
        else paths.push_back(argv[i]);
    }
    const int n = (int)paths.size();
    if (n == 0) {
        usage();
        return 2;
    }
    std::vector<std::vector<uint8_t>> data(n);
    std::vector<std::string> error(n);
    std::vector<lacx_spectrum> spec(n, lacx_spectrum{});
    std::vector<std::vector<lacx_spectrum_row>> rows(n);
    std::vector<int> lacs, wavs;  // indices of the files of each kind that go to the device
    std::vector<lacx_wav_info> winfo(n, lacx_wav_info{});
    for (int i = 0; i < n; ++i) {
        if (!load_file(paths[i], data[i])) {
            error[i] = "Failed to read file";
        } else if (data[i].size() >= 4 && std::memcmp(data[i].data(), "RIFF", 4) == 0) {
            if (lacx_wav_parse(data[i].data(), data[i].size(), &winfo[i]) != LACX_OK) error[i] = "Failed to read WAV";
            else wavs.push_back(i);
        } else {
            lacs.push_back(i);
        }
    }
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 2;
    }
    auto collect = [&](const std::vector<int>& which, int rc, const std::vector<int>& item_rc, const std::vector<lacx_spectrum>& out) {
        for (size_t k = 0; k < which.size(); ++k) {
            const lacx_spectrum_row* r = nullptr;
            uint32_t count = 0;
            if (rc != LACX_E_DEVICE && item_rc[k] == LACX_OK && (rc == LACX_OK || out[k].window) && lacx_decoder_item_spectrum_rows(dec, (uint32_t)k, &r, &count) == LACX_OK) {
                spec[which[k]] = out[k];
                rows[which[k]].assign(r, r + count);
            } else {
                error[which[k]] = rc == LACX_E_DEVICE || item_rc[k] == LACX_OK ? lacx_decode_last_error() : lacx_decoder_item_error(dec, (uint32_t)k);
            }
        }
    };
    if (!lacs.empty()) {
        std::vector<lacx_span> spans;
        for (int i : lacs) spans.push_back(lacx_span{data[i].data(), data[i].size()});
        std::vector<int> item_rc(lacs.size(), LACX_OK);
        std::vector<lacx_spectrum> out(lacs.size());
        const int rc = lacx_decoder_spectrum_batch_device(dec, spans.data(), (uint32_t)spans.size(), window, floor_db, nullptr, item_rc.data(), out.data(), nullptr);
        collect(lacs, rc, item_rc, out);
    }
    if (!wavs.empty()) {
        std::vector<lacx_digest_source> src;
        std::vector<void*> dev;
        std::vector<int> sent;
        for (int i : wavs) {
            const lacx_wav_info& w = winfo[i];
            const uint64_t bytes = w.frames * w.channels * (uint64_t)(w.bit_depth / 8);
            void* p = nullptr;
            if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess ||
                hipMemcpy(p, data[i].data() + w.data_offset, bytes, hipMemcpyHostToDevice) != hipSuccess) {
                error[i] = "Failed to upload WAV data to the device";
                if (p) (void)hipFree(p);
                continue;
            }
            lacx_digest_source s{};
            s.pcm = lacx_pcm{p, nullptr, w.bit_depth == 16 ? LACX_PCM_INTERLEAVED_I16 : LACX_PCM_INTERLEAVED_I24, w.channels};
            s.frames = w.frames;
            s.sample_rate = w.sample_rate;
            s.bit_depth = (uint8_t)w.bit_depth;
            src.push_back(s), dev.push_back(p), sent.push_back(i);
        }
        if (!src.empty()) {
            std::vector<int> item_rc(src.size(), LACX_OK);
            std::vector<lacx_spectrum> out(src.size());
            const int rc = lacx_decoder_spectrum_pcm_batch_device(dec, src.data(), (uint32_t)src.size(), window, floor_db, nullptr, item_rc.data(), out.data(), nullptr);
            collect(sent, rc, item_rc, out);
        }
        for (void* p : dev) (void)hipFree(p);
    }
    bool refused = false;
    for (int i = 0; i < n; ++i) {
        if (error[i].empty()) continue;
        std::cerr << "Spectrum failed: " << paths[i] << ": " << error[i] << "\n";
        refused = true;
    }
    lacx_decoder_destroy(dec);
    if (refused) return 2;
    for (int i = 0; i < n; ++i) {
        std::cout << spectrum_text(spec[i]) << " " << paths[i] << "\n";
        for (size_t s = 0; per_block && s < rows[i].size(); ++s)
            for (unsigned c = 0; c < spec[i].channels; ++c) {
                std::string line = "  row=" + std::to_string(s) + " ch" + std::to_string(c) + ":";
                for (int b = 0; b < 64; ++b) {
                    char v[40];
                    std::snprintf(v, sizeof(v), " %.17g", rows[i][s].power[c][b]);
                    line += v;
                }
                std::cout << line << "\n";
            }
    }
    return 0;
}

// lacx_cli accuraterip FILE... [--tracks=n0,n1,...] [--radius=N] [--not-first] [--not-last] [--lba0=N] [--match=HEX[,HEX...]]:
// the files, .lac and WAV, are together one disc of CD audio in argument order.  All .lac: one stream job
// (lacx_decoder_accuraterip_batch_device).  Otherwise every .lac is decoded to its WAV image first and the data chunks go to
// the device as one source job (lacx_decoder_accuraterip_pcm_batch_device): the same sums either way.  Prints the ids, then per
// track `NN start frames v1 v2 s450` at offset 0 (sums in hex), then with --match one line per (track, offset, kind) whose sum
// is one of the values.  Exit 0 done, 1 with --match when nothing matched, 2 refused (the message on stderr).
int accuraterip_command(int argc, char** argv) {
    std::vector<const char*> paths;
    std::vector<uint64_t> tracks;
    std::vector<uint32_t> match;
    bool matching = false;
    lacx_ar_disc disc{};
    disc.flags = LACX_AR_FIRST | LACX_AR_LAST;
    auto numbers = [](const char* text, int base, auto& out) {
        for (const char* p = text; *p;) {
            char* end = nullptr;
            const unsigned long long v = std::strtoull(p, &end, base);
            if (end == p || (*end && *end != ',')) return false;
            out.push_back((typename std::remove_reference_t<decltype(out)>::value_type)v);
            p = *end ? end + 1 : end;
        }
        return !out.empty();
    };
    bool bad_option = false;
    for (int i = 2; i < argc; ++i) {
        const char* a = argv[i];
        std::vector<uint64_t> one;
        if (std::strncmp(a, "--tracks=", 9) == 0) bad_option |= !numbers(a + 9, 10, tracks);
        else if (std::strncmp(a, "--radius=", 9) == 0) bad_option |= !numbers(a + 9, 10, one) || one.size() != 1 || (disc.radius = (uint32_t)one[0], one[0] >> 32);
        else if (std::strncmp(a, "--lba0=", 7) == 0) bad_option |= !numbers(a + 7, 10, one) || one.size() != 1 || (disc.lba0 = (uint32_t)one[0], one[0] >> 32);
        else if (std::strncmp(a, "--match=", 8) == 0) matching = true, bad_option |= !numbers(a + 8, 16, match);
        else if (std::strcmp(a, "--not-first") == 0) disc.flags &= ~LACX_AR_FIRST;
        else if (std::strcmp(a, "--not-last") == 0) disc.flags &= ~LACX_AR_LAST;
        else if (std::strncmp(a, "--", 2) == 0) bad_option = true;
        else paths.push_back(a);
    }
    const int n = (int)paths.size();
    if (n == 0 || bad_option) {
        usage();
        return 2;
    }
    std::vector<std::vector<uint8_t>> data(n);
    bool all_lac = true;
    for (int i = 0; i < n; ++i) {
        if (!load_file(paths[i], data[i])) {
            std::cerr << "AccurateRip failed: " << paths[i] << ": Failed to read file\n";
            return 2;
        }
        if (data[i].size() >= 4 && std::memcmp(data[i].data(), "RIFF", 4) == 0) all_lac = false;
    }
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 2;
    }
    disc.first_source = 0, disc.sources = (uint32_t)n, disc.first_track = 0, disc.tracks = (uint32_t)tracks.size();
    lacx_ar_result res{};
    int rc = LACX_OK, disc_rc = LACX_OK;
    std::vector<void*> dev;
    std::string why;
    if (all_lac) {
        std::vector<lacx_span> spans;
        for (int i = 0; i < n; ++i) spans.push_back(lacx_span{data[i].data(), data[i].size()});
        rc = lacx_decoder_accuraterip_batch_device(dec, spans.data(), (uint32_t)n, tracks.data(), (uint32_t)tracks.size(), &disc, 1, nullptr, &disc_rc, &res, nullptr);
    } else {
        std::vector<lacx_digest_source> src;
        for (int i = 0; i < n && why.empty(); ++i) {
            if (data[i].size() < 4 || std::memcmp(data[i].data(), "RIFF", 4) != 0) {  // a .lac among WAV files: its WAV image
                uint8_t* img = nullptr;
                uint64_t size = 0;
                if (lacx_decoder_decode_wav(dec, data[i].data(), data[i].size(), &img, &size, nullptr) != LACX_OK) {
                    why = std::string(paths[i]) + ": " + lacx_decode_last_error();
                    break;
                }
                data[i].assign(img, img + size);
                lacx_free(img);
            }
            lacx_wav_info w{};
            if (lacx_wav_parse(data[i].data(), data[i].size(), &w) != LACX_OK) {
                why = std::string(paths[i]) + ": Failed to read WAV";
                break;
            }
            const uint64_t bytes = w.frames * w.channels * (uint64_t)(w.bit_depth / 8);
            void* p = nullptr;
            if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess || hipMemcpy(p, data[i].data() + w.data_offset, bytes, hipMemcpyHostToDevice) != hipSuccess) {
                why = std::string(paths[i]) + ": Failed to upload WAV data to the device";
                if (p) (void)hipFree(p);
                break;
            }
            dev.push_back(p);
            lacx_digest_source x{};
            x.pcm = lacx_pcm{p, nullptr, w.bit_depth == 16 ? LACX_PCM_INTERLEAVED_I16 : LACX_PCM_INTERLEAVED_I24, w.channels};
            x.frames = w.frames, x.sample_rate = w.sample_rate, x.bit_depth = (uint8_t)w.bit_depth;
            src.push_back(x);
        }
        if (why.empty())
            rc = lacx_decoder_accuraterip_pcm_batch_device(dec, src.data(), (uint32_t)n, tracks.data(), (uint32_t)tracks.size(), &disc, 1, nullptr, &disc_rc, &res, nullptr);
    }
    if (why.empty() && rc != LACX_OK) why = disc_rc != LACX_OK && rc != LACX_E_DEVICE ? lacx_decoder_item_error(dec, 0) : lacx_decode_last_error();
    int code = 0;
    if (!why.empty()) {
        std::cerr << "AccurateRip failed: " << why << "\n";
        code = 2;
    } else {
        const lacx_ar_track* tr = nullptr;
        uint32_t count = 0;
        (void)lacx_decoder_item_ar_tracks(dec, 0, &tr, &count);
        char line[192];
        std::snprintf(line, sizeof(line), "id1=%08x id2=%08x cddb=%08x tracks=%u frames=%llu radius=%u", res.ids.id1, res.ids.id2, res.ids.cddb, res.tracks,
                      (unsigned long long)res.frames, res.radius);
        std::cout << line << (res.flags & LACX_AR_NO_IDS ? " no-ids" : "") << "\n";
        for (uint32_t t = 0; t < count; ++t) {
            std::snprintf(line, sizeof(line), "%02u %llu %llu %08x %08x %08x", t + 1, (unsigned long long)tr[t].start, (unsigned long long)tr[t].frames, tr[t].v1,
                          tr[t].v2, tr[t].s450);
            std::cout << line << (tr[t].flags & LACX_AR_TRACK_SHORT ? " short" : "") << (tr[t].flags & LACX_AR_TRACK_NO_S450 ? " no-s450" : "") << "\n";
        }
        size_t found = 0;
        for (uint32_t t = 0; matching && t < count; ++t) {
            const uint32_t* sums[3] = {nullptr, nullptr, nullptr};
            uint32_t width = 0;
            if (lacx_decoder_item_ar_sums(dec, 0, t, &sums[0], &sums[1], &sums[2], &width) != LACX_OK) continue;
            const char* kind[3] = {"v1", "v2", "s450"};
            for (uint32_t k = 0; k < width; ++k)
                for (int q = 0; q < 3; ++q) {
                    if ((q == 2 && (tr[t].flags & LACX_AR_TRACK_NO_S450)) || (q < 2 && (tr[t].flags & LACX_AR_TRACK_SHORT))) continue;
                    if (std::find(match.begin(), match.end(), sums[q][k]) == match.end()) continue;
                    std::snprintf(line, sizeof(line), "match track=%02u offset=%d kind=%s value=%08x", t + 1, (int)k - (int)res.radius, kind[q], sums[q][k]);
                    std::cout << line << "\n";
                    ++found;
                }
        }
        if (matching && !found) code = 1;
    }
    for (void* p : dev) (void)hipFree(p);
    lacx_decoder_destroy(dec);
    return code;
}

// lacx_cli compare A B [--radius=N] [--centre=N] [--blocks] [--offsets]: A and B each a .lac or a WAV.  Both .lac: one stream
// job (lacx_decoder_compare_batch_device).  Otherwise the source form (lacx_decoder_compare_pcm_batch_device): a .lac is first
// decoded into planar int32 on the device (lacx_decoder_decode_batch_device), a WAV's data chunk goes there as it is: the same
// answer either way.  Prints `offset=O identical ...` or `offset=O mismatches=N (left[, right]) first=T last=T peak=P (dBFS) ch=C
// at=T rms=dBFS`, then frames, rows, lead and tail; times as frames on A's axis and seconds.  Exit 0 no sample differs at the
// chosen offset, 1 they differ, 2 refused (the message on stderr).
int compare_command(int argc, char** argv) {
    std::vector<const char*> paths;
    lacx_compare_pair pair{};
    bool blocks = false, offsets = false, bad_option = false;
    for (int i = 2; i < argc; ++i) {
        const char* a = argv[i];
        char* end = nullptr;
        if (std::strncmp(a, "--radius=", 9) == 0) {
            const unsigned long long v = std::strtoull(a + 9, &end, 10);
            bad_option |= end == a + 9 || *end || v >> 32;
            pair.radius = (uint32_t)v;
        } else if (std::strncmp(a, "--centre=", 9) == 0) {
            pair.centre = std::strtoll(a + 9, &end, 10);
            bad_option |= end == a + 9 || *end;
        } else if (std::strcmp(a, "--blocks") == 0) blocks = true;
        else if (std::strcmp(a, "--offsets") == 0) offsets = true;
        else if (std::strncmp(a, "--", 2) == 0) bad_option = true;
        else paths.push_back(a);
    }
    if (paths.size() != 2 || bad_option) {
        usage();
        return 2;
    }
    std::vector<uint8_t> data[2];
    bool all_lac = true;
    for (int i = 0; i < 2; ++i) {
        if (!load_file(paths[i], data[i])) {
            std::cerr << "Compare failed: " << paths[i] << ": Failed to read file\n";
            return 2;
        }
        if (data[i].size() >= 4 && std::memcmp(data[i].data(), "RIFF", 4) == 0) all_lac = false;
    }
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 2;
    }
    pair.a = 0, pair.b = 1;
    lacx_compare res{};
    int rc = LACX_OK, pair_rc = LACX_OK;
    std::vector<void*> dev;
    std::string why;
    if (all_lac) {
        const lacx_span spans[2] = {{data[0].data(), data[0].size()}, {data[1].data(), data[1].size()}};
        rc = lacx_decoder_compare_batch_device(dec, spans, 2, &pair, 1, nullptr, &pair_rc, &res, nullptr);
    } else {
        lacx_digest_source src[2]{};
        auto device = [&](uint64_t bytes, const void* from) -> void* {
            void* p = nullptr;
            if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
            dev.push_back(p);
            if (from && hipMemcpy(p, from, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
            return p;
        };
        for (int i = 0; i < 2 && why.empty(); ++i) {
            lacx_digest_source& x = src[i];
            if (data[i].size() < 4 || std::memcmp(data[i].data(), "RIFF", 4) != 0) {  // a .lac beside a WAV: decoded into planar int32
                lacx_stream_info f{};
                if (lacx_stream_parse(data[i].data(), data[i].size(), &f) != LACX_OK) {
                    why = std::string(paths[i]) + ": " + lacx_decode_last_error();
                    break;
                }
                int32_t* l = static_cast<int32_t*>(device(4 * f.frames, nullptr));
                int32_t* r = f.channels == 2 ? static_cast<int32_t*>(device(4 * f.frames, nullptr)) : nullptr;
                if (!l || (f.channels == 2 && !r)) {
                    why = std::string(paths[i]) + ": Failed to allocate on the device";
                    break;
                }
                const lacx_decode_item item{data[i].data(), data[i].size(), l, r, f.frames};
                if (lacx_decoder_decode_batch_device(dec, &item, 1, nullptr, nullptr, nullptr) != LACX_OK) {
                    why = std::string(paths[i]) + ": " + lacx_decode_last_error();
                    break;
                }
                x.pcm = lacx_pcm{l, r, LACX_PCM_PLANAR_I32, f.channels};
                x.frames = f.frames, x.sample_rate = f.sample_rate, x.bit_depth = (uint8_t)f.bit_depth;
                continue;
            }
            lacx_wav_info w{};
            if (lacx_wav_parse(data[i].data(), data[i].size(), &w) != LACX_OK) {
                why = std::string(paths[i]) + ": Failed to read WAV";
                break;
            }
            const uint64_t bytes = w.frames * w.channels * (uint64_t)(w.bit_depth / 8);
            void* p = device(bytes, data[i].data() + w.data_offset);
            if (!p) {
                why = std::string(paths[i]) + ": Failed to upload WAV data to the device";
                break;
            }
            x.pcm = lacx_pcm{p, nullptr, w.bit_depth == 16 ? LACX_PCM_INTERLEAVED_I16 : LACX_PCM_INTERLEAVED_I24, w.channels};
            x.frames = w.frames, x.sample_rate = w.sample_rate, x.bit_depth = (uint8_t)w.bit_depth;
        }
        if (why.empty()) rc = lacx_decoder_compare_pcm_batch_device(dec, src, 2, &pair, 1, nullptr, &pair_rc, &res, nullptr);
    }
    if (why.empty() && rc != LACX_OK) why = pair_rc != LACX_OK && rc != LACX_E_DEVICE ? lacx_decoder_item_error(dec, 0) : lacx_decode_last_error();
    int code = 0;
    if (!why.empty()) {
        std::cerr << "Compare failed: " << why << "\n";
        code = 2;
    } else {
        char line[320];
        const double rate = res.sample_rate ? (double)res.sample_rate : 1.0, full = (double)(1u << (res.bit_depth - 1));
        const char* side[3] = {"-", "A", "B"};
        if (res.mismatches == 0) {
            std::snprintf(line, sizeof(line), "offset=%lld identical", (long long)res.offset);
        } else {
            code = 1;
            char per[64];
            if (res.channels == 2) std::snprintf(per, sizeof(per), "%llu, %llu", (unsigned long long)res.ch[0].mismatches, (unsigned long long)res.ch[1].mismatches);
            else std::snprintf(per, sizeof(per), "%llu", (unsigned long long)res.ch[0].mismatches);
            const long double sq = (long double)res.sum_sq_hi * 18446744073709551616.0L + (long double)res.sum_sq_lo;
            const double rms = std::sqrt((double)(sq / ((long double)res.domain_frames * res.channels))) / full;
            std::snprintf(line, sizeof(line), "offset=%lld mismatches=%llu (%s) first=%lld (%.6f s) last=%lld (%.6f s) peak=%u (%.2f dBFS) ch=%u at=%lld (%.6f s) rms=%.2f dBFS",
                          (long long)res.offset, (unsigned long long)res.mismatches, per, (long long)res.first, (double)res.first / rate, (long long)res.last,
                          (double)res.last / rate, res.peak, 20.0 * std::log10((double)res.peak / full), (unsigned)res.peak_channel, (long long)res.peak_at,
                          (double)res.peak_at / rate, 20.0 * std::log10(rms));
        }
        std::cout << line;
        std::snprintf(line, sizeof(line), " frames=%llu,%llu domain=%lld+%llu rows=%llu differing_rows=%llu lead=%llu (%s) tail=%llu (%s)", (unsigned long long)res.frames_a,
                      (unsigned long long)res.frames_b, (long long)res.domain_first, (unsigned long long)res.domain_frames, (unsigned long long)res.rows,
                      (unsigned long long)res.rows_differ, (unsigned long long)res.lead, side[res.lead_side % 3], (unsigned long long)res.tail, side[res.tail_side % 3]);
        std::cout << line << "\n";
        if (offsets) {
            const uint64_t* counts = nullptr;
            uint32_t n = 0;
            (void)lacx_decoder_item_compare_counts(dec, 0, &counts, &n);
            for (uint32_t k = 0; k < n; ++k) std::cout << "o=" << (long long)pair.centre - (long long)pair.radius + (long long)k << " " << counts[k] << "\n";
        }
        if (blocks) {
            const lacx_compare_row* rows = nullptr;
            uint32_t n = 0;
            (void)lacx_decoder_item_compare_rows(dec, 0, &rows, &n);
            for (uint32_t r = 0; r < n; ++r) {
                std::cout << "row " << r;
                for (uint32_t c = 0; c < res.channels; ++c) {
                    const lacx_compare_channel_row& x = rows[r].ch[c];
                    if (!x.mismatches) std::cout << " | 0";
                    else
                        std::cout << " | " << x.mismatches << " first=" << (long long)(res.domain_first + (int64_t)x.first) << " last=" << (long long)(res.domain_first + (int64_t)x.last)
                                  << " peak=" << x.max_abs << " at=" << (long long)(res.domain_first + (int64_t)x.max_at) << " sum_abs=" << x.sum_abs << " sum_sq=" << x.sum_sq;
                }
                std::cout << "\n";
            }
        }
    }
    for (void* p : dev) (void)hipFree(p);
    lacx_decoder_destroy(dec);
    return code;
}

// lacx_cli inspect FILE... [--blocks] [--partitions]: how every .lac was coded and where its bits go, read out of the bytes
// on the device by a parse-only walk (lacx_decoder_inspect_batch_device), all files as one job.  One line of integers per
// file in argument order; with --blocks one further line per block (its channel blocks behind it), with --partitions one
// per partition: mode, table k, bits.  Lenient like stats: a damaged or truncated stream prints its line with lost_blocks
// counted.  Exit 0 when every file was inspected; otherwise the refused files' messages on stderr and exit 1.
int inspect_command(int argc, char** argv) {
    bool per_block = false, per_part = false;
    std::vector<const char*> paths;
    for (int i = 2; i < argc; ++i) {
        if (std::strcmp(argv[i], "--blocks") == 0) per_block = true;
        else if (std::strcmp(argv[i], "--partitions") == 0) per_part = true;
        else if (std::strncmp(argv[i], "--", 2) == 0) {
            std::cerr << "Error: unknown option " << argv[i] << "\n";
            usage();
            return 1;
        } else paths.push_back(argv[i]);
    }
    const int n = (int)paths.size();
    if (n == 0) {
        usage();
        return 1;
    }
    std::vector<std::vector<uint8_t>> data(n);
    std::vector<std::string> error(n);
    std::vector<int> sent;
    std::vector<lacx_span> spans;
    for (int i = 0; i < n; ++i) {
        if (!load_file(paths[i], data[i])) error[i] = "Failed to read file";
        else sent.push_back(i), spans.push_back(lacx_span{data[i].data(), data[i].size()});
    }
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 1;
    }
    std::vector<lacx_stream_report> out(spans.size());
    std::vector<int> item_rc(spans.size(), LACX_OK);
    int rc = LACX_OK;
    if (!spans.empty())
        rc = lacx_decoder_inspect_batch_device(dec, spans.data(), (uint32_t)spans.size(), per_part ? LACX_INSPECT_PARTITIONS : 0u, nullptr,
                                               item_rc.data(), out.data(), nullptr);
    int status = 0;
    size_t k = 0;
    for (int i = 0; i < n; ++i) {
        if (error[i].empty()) {
            if (item_rc[k] != LACX_OK) error[i] = lacx_decoder_item_error(dec, (uint32_t)k);  // (a failure of the whole call is every item's)
            else if (rc == LACX_E_DEVICE) error[i] = lacx_decode_last_error();
            ++k;
        }
        if (!error[i].empty()) {
            std::cerr << "Inspect failed: " << paths[i] << ": " << error[i] << "\n";
            status = 1;
            continue;
        }
        const uint32_t item = (uint32_t)(k - 1);
        const lacx_stream_report& t = out[item];
        std::cout << "frames=" << t.frames << " channels=" << (unsigned)t.channels << " bits=" << (unsigned)t.bit_depth << " rate=" << t.sample_rate
                  << " version=" << (unsigned)t.version << " stereo_mode=" << (unsigned)t.stereo_mode << " blocks=" << t.blocks
                  << " lost_blocks=" << t.lost_blocks << " head_bytes=" << t.head_bytes << " payload_bytes=" << t.payload_bytes
                  << " ms_blocks=" << t.ms_blocks << " channel_blocks=" << t.channel_blocks << " fixed=";
        for (int o = 0; o < 5; ++o) std::cout << (o ? "," : "") << t.fixed_blocks[o];
        std::cout << " fir=" << t.fir_blocks << " lpc=";
        for (int o = 1; o <= 32; ++o) std::cout << (o > 1 ? "," : "") << t.lpc_blocks[o];
        std::cout << " partition_orders=";
        for (int p = 0; p < 9; ++p) std::cout << (p ? "," : "") << t.partition_order_blocks[p];
        std::cout << " mode_parts=" << t.mode_parts[0] << "," << t.mode_parts[1] << "," << t.mode_parts[2] << "," << t.mode_parts[3]
                  << " mode_samples=" << t.mode_samples[0] << "," << t.mode_samples[1] << "," << t.mode_samples[2] << "," << t.mode_samples[3]
                  << " flag_bits=" << t.flag_bits << " header_bits=" << t.header_bits << " tag_bits=" << t.tag_bits << " unary_bits=" << t.unary_bits
                  << " remainder_bits=" << t.remainder_bits << " escape_bits=" << t.escape_bits << " pad_bits=" << t.pad_bits
                  << " rice_samples=" << t.rice_samples << " run_tokens=" << t.run_tokens << " run_samples=" << t.run_samples
                  << " escape_samples=" << t.escape_samples << " bin_samples=" << t.bin_samples[0] << "," << t.bin_samples[1] << "," << t.bin_samples[2]
                  << " sum_u=" << dec128(t.sum_u_lo, t.sum_u_hi, false) << " max_u=" << t.max_u << " unary_max=" << t.unary_max
                  << " k_min=" << (unsigned)t.k_min << " k_max=" << (unsigned)t.k_max << " " << paths[i] << "\n";
        const lacx_block_info* rows = nullptr;
        uint32_t count = 0;
        if ((per_block || per_part) && lacx_decoder_item_block_info(dec, item, &rows, &count) != LACX_OK) count = 0;
        for (uint32_t b = 0; b < count; ++b) {
            const lacx_block_info& r = rows[b];
            if (per_block) {
                std::cout << "  block=" << b << " frames=" << r.frames << " bytes=" << r.bytes << " code=" << r.code << " ms=" << (unsigned)r.ms;
                for (uint32_t c = 0; c < r.channels; ++c) {
                    const lacx_channel_info& s = r.ch[c];
                    std::cout << " ch" << c << ": type=" << (unsigned)s.predictor_type << " order=" << (unsigned)s.order
                              << " partition_order=" << (unsigned)s.partition_order << " bits=" << s.bits << " header=" << s.header_bits
                              << " tag=" << s.tag_bits << " unary=" << s.unary_bits << " remainder=" << s.remainder_bits << " escape=" << s.escape_bits
                              << " pad=" << s.pad_bits << " rice=" << s.rice_samples << " runs=" << s.run_tokens << " run_samples=" << s.run_samples
                              << " escapes=" << s.escape_samples << " bins=" << s.bin_samples[0] << "," << s.bin_samples[1] << "," << s.bin_samples[2]
                              << " k=" << (unsigned)s.k_min << ".." << (unsigned)s.k_max << " unary_max=" << s.unary_max << " max_u=" << s.max_u
                              << " sum_u=" << (unsigned long long)s.sum_u;
                }
                std::cout << "\n";
            }
            for (uint32_t c = 0; per_part && c < r.channels; ++c) {
                const uint8_t* mk = nullptr;
                const uint32_t* pb = nullptr;
                uint32_t parts = 0;
                if (lacx_decoder_item_partitions(dec, item, b, c, &mk, &pb, &parts) != LACX_OK) continue;
                for (uint32_t p = 0; p < parts; ++p)
                    std::cout << "    block=" << b << " ch=" << c << " partition=" << p << " mode=" << (mk[p] >> 5) << " k=" << (mk[p] & 31u)
                              << " bits=" << pb[p] << "\n";
            }
        }
    }
    lacx_decoder_destroy(dec);
    return status;
}

// The canonical WAV image of planar PCM (the source form lacx_decoder_verify_wav takes).
std::vector<uint8_t> wav_image(const std::vector<int32_t>& left, const std::vector<int32_t>* right, uint32_t rate, uint32_t bits) {
    const uint32_t ch = right ? 2u : 1u, bps = bits / 8u, align = ch * bps;
    const uint64_t data = (uint64_t)left.size() * align;
    std::vector<uint8_t> w(44 + data + (data & 1u), 0);
    auto u16 = [&](size_t at, uint32_t v) { w[at] = (uint8_t)v, w[at + 1] = (uint8_t)(v >> 8); };
    auto u32 = [&](size_t at, uint32_t v) { u16(at, v & 0xFFFFu), u16(at + 2, v >> 16); };
    std::memcpy(&w[0], "RIFF", 4);
    u32(4, (uint32_t)(36u + data + (data & 1u)));
    std::memcpy(&w[8], "WAVEfmt ", 8);
    u32(16, 16), u16(20, 1), u16(22, ch), u32(24, rate), u32(28, rate * align), u16(32, align), u16(34, bits);
    std::memcpy(&w[36], "data", 4);
    u32(40, (uint32_t)data);
    uint8_t* p = &w[44];
    for (size_t i = 0; i < left.size(); ++i)
        for (uint32_t c = 0; c < ch; ++c) {
            const uint32_t v = (uint32_t)(c ? (*right)[i] : left[i]);
            for (uint32_t k = 0; k < bps; ++k) *p++ = (uint8_t)(v >> (8u * k));
        }
    return w;
}

// lacx_cli selftest (ref src/main.cpp:803-909)
int selftest_command() {
    const double pi = 3.14159265358979323846;
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 1;
    }
    struct Run {
        std::vector<uint8_t> lac;
        lacx_stream_info info{};
        long long verify_us = 0;
    };
    // one encode, verified on the device against its source; false after printing why
    auto roundtrip = [&](const char* what, uint32_t rate, uint8_t depth, uint8_t mode, const std::vector<int32_t>& left,
                         const std::vector<int32_t>* right, Run& out) -> bool {
        lacx_config cfg{};
        cfg.sample_rate = rate, cfg.bit_depth = depth, cfg.stereo_mode = mode;
        cfg.zero_run_enabled = 1, cfg.partitioning_enabled = 1, cfg.device = -1;
        lacx_encoder* enc = nullptr;
        if (lacx_encoder_create(&cfg, &enc) != LACX_OK) {
            std::cerr << "Error: lacx_encoder_create failed\n";
            return false;
        }
        uint8_t* bytes = nullptr;
        uint64_t size = 0;
        if (lacx_encode(enc, left.data(), right ? right->data() : nullptr, left.size(), &bytes, &size) != LACX_OK) {
            std::cerr << "Error: " << lacx_last_error(enc) << "\n";
            lacx_encoder_destroy(enc);
            return false;
        }
        out.lac.assign(bytes, bytes + size);
        lacx_free(bytes);
        lacx_encoder_destroy(enc);
        const std::vector<uint8_t> wav = wav_image(left, right, rate, depth);
        lacx_verify_result res{};
        const auto t0 = std::chrono::high_resolution_clock::now();
        const int rc = lacx_decoder_verify_wav(dec, out.lac.data(), out.lac.size(), wav.data(), wav.size(), &res, nullptr);
        const auto t1 = std::chrono::high_resolution_clock::now();
        out.verify_us = std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
        if (rc != LACX_OK) {
            std::cerr << what << " roundtrip mismatch for sr=" << rate << " depth=" << int(depth) << ": " << lacx_decode_last_error() << "\n";
            return false;
        }
        if (lacx_stream_parse(out.lac.data(), out.lac.size(), &out.info) != LACX_OK) {
            std::cerr << what << " header unreadable: " << lacx_decode_last_error() << "\n";
            return false;
        }
        return true;
    };
    auto run_pair = [&](uint32_t rate, uint8_t depth) -> bool {
        const size_t frames = std::max<size_t>(rate / 20, 2048);
        std::vector<int32_t> left(frames), right(frames);
        const int64_t amplitude = depth == 24 ? (int64_t)0x7FFFFF / 3 : (int64_t)30000;
        for (size_t i = 0; i < frames; ++i) {
            const double t = (double)i / (double)rate;
            left[i] = (int32_t)(std::sin(2.0 * pi * 440.0 * t) * amplitude);
            right[i] = (int32_t)(std::sin(2.0 * pi * 443.0 * t) * (amplitude * 0.95));
        }
        Run lr, ms, au, mono;
        if (!roundtrip("LR", rate, depth, 0, left, &right, lr)) return false;
        if (lr.info.sample_rate != rate || lr.info.bit_depth != depth) {
            std::cerr << "LR header mismatch sr=" << lr.info.sample_rate << " depth=" << int(lr.info.bit_depth) << "\n";
            return false;
        }
        if (!roundtrip("MS", rate, depth, 1, left, &right, ms)) return false;
        if (ms.info.sample_rate != rate || ms.info.bit_depth != depth) {
            std::cerr << "MS header mismatch sr=" << ms.info.sample_rate << " depth=" << int(ms.info.bit_depth) << "\n";
            return false;
        }
        if (!roundtrip("Auto-stereo", rate, depth, 2, left, &right, au)) return false;
        if (au.info.stereo_mode != 2) {
            std::cerr << "Auto-stereo header mismatch stereo_mode=" << int(au.info.stereo_mode) << "\n";
            return false;
        }
        if (!roundtrip("Mono", rate, depth, 0, left, nullptr, mono)) return false;
        if (mono.info.channels != 1) {
            std::cerr << "Mono header mismatch channels=" << int(mono.info.channels) << "\n";
            return false;
        }
        std::cout << "Selftest sr=" << rate << "Hz depth=" << int(depth) << " LR=" << lr.lac.size() << " bytes (" << lr.verify_us
                  << "us decode) MS=" << ms.lac.size() << " bytes (" << ms.verify_us << "us decode) -> MS is "
                  << (ms.lac.size() < lr.lac.size() ? "smaller" : "not smaller") << "\n";
        return true;
    };
    const bool ok = run_pair(44100, 16) && run_pair(48000, 24) && run_pair(96000, 24) && run_pair(192000, 24);
    lacx_decoder_destroy(dec);
    if (!ok) return 1;
    std::cout << "Selftest complete: adaptive block tests passed.\n";
    return 0;
}

// recompress / cut / join: one output of lacx_transcode_batch over the input files.  Exit 0 done, 1 the new stream does not
// decode to its sources (--verify), 2 refused; the output is published only on success.
int transcode_command(const std::string& mode, int argc, char** argv) {
    std::vector<std::string> in_paths;
    std::string out_path;
    int first_flag = 4;
    if (mode == "join") {
        out_path = argv[2];
        for (first_flag = 3; first_flag < argc && std::string(argv[first_flag]).compare(0, 2, "--") != 0; ++first_flag) in_paths.push_back(argv[first_flag]);
    } else {
        in_paths.push_back(argv[2]);
        out_path = argv[3];
    }
    lacx_edit_output o{};
    o.stereo_mode = 2;
    uint64_t start = 0, frames = LACX_TO_END;
    bool verify = false, zero_run = true, partitioning = true, have_start = false;
    const bool re = mode == "recompress", cut = mode == "cut";
    auto number = [](const std::string& v, uint64_t& out) {
        if (v.empty() || v.size() > 18) return false;
        for (char c : v)
            if (c < '0' || c > '9') return false;
        out = std::stoull(v);
        return true;
    };
    for (int i = first_flag; i < argc; ++i) {
        const std::string flag = argv[i];
        static const char* const kOps[] = {"keep", "left", "right", "fold", "swap", "dual"};
        bool ok = flag == "--verify";
        if (ok) verify = true;
        if (re && flag == "--stereo=lr") ok = true, o.stereo_mode = 0;
        if (re && flag == "--stereo=ms") ok = true, o.stereo_mode = 1;
        if (re && flag == "--stereo=auto") ok = true, o.stereo_mode = 2;
        if (re && flag == "--no-zero-run") ok = true, zero_run = false;
        if (re && flag == "--no-partitioning") ok = true, partitioning = false;
        if (re && flag == "--depth=16") ok = true, o.bit_depth = 16;
        if (re && flag == "--depth=24") ok = true, o.bit_depth = 24;
        for (uint8_t c = 0; re && c < 6; ++c)
            if (flag == std::string("--channels=") + kOps[c]) ok = true, o.channel_op = c;
        if (cut && flag.compare(0, 8, "--start=") == 0) ok = have_start = number(flag.substr(8), start);
        if (cut && flag.compare(0, 9, "--frames=") == 0) ok = number(flag.substr(9), frames);
        if (!ok) {
            usage();
            return 2;
        }
    }
    if (in_paths.empty() || (cut && !have_start)) {
        usage();
        return 2;
    }
    std::vector<std::vector<uint8_t>> files(in_paths.size());
    std::vector<lacx_edit_segment> segs;
    for (size_t i = 0; i < in_paths.size(); ++i) {
        if (same_file(in_paths[i], out_path)) {
            std::cerr << "Input and output paths must be different\n";
            return 2;
        }
        if (!load_file(in_paths[i], files[i])) {
            std::cerr << "Failed to read LAC file: " << in_paths[i] << "\n";
            return 2;
        }
        segs.push_back(lacx_edit_segment{files[i].data(), files[i].size(), start, frames});
    }
    o.first_segment = 0;
    o.segments = (uint32_t)segs.size();
    lacx_config cfg{};
    cfg.sample_rate = 48000;  // (the outputs' formats come from their sources)
    cfg.bit_depth = 16;
    cfg.zero_run_enabled = zero_run ? 1 : 0;
    cfg.partitioning_enabled = partitioning ? 1 : 0;
    cfg.device = -1;
    lacx_encoder* enc = nullptr;
    lacx_decoder* dec = nullptr;
    if (lacx_encoder_create(&cfg, &enc) != LACX_OK || lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: cannot create the encoder and the decoder\n";
        if (enc) lacx_encoder_destroy(enc);
        return 2;
    }
    lacx_span out{};
    lacx_edit_result res{};
    const int rc = lacx_transcode_batch(dec, enc, segs.data(), (uint32_t)segs.size(), &o, 1, verify ? LACX_TRANSCODE_VERIFY : 0u, &out, nullptr, &res, nullptr);
    int status = rc == LACX_OK ? 0 : rc == LACX_E_MISMATCH ? 1 : 2;
    if (status == 2) std::cerr << (rc == LACX_E_INVALID ? "Refused: " : "Error: ") << lacx_decode_last_error() << "\n";  // (no device, a failed decode)
    if (status == 1) std::cerr << "Verify failed: " << lacx_decode_last_error() << "\n";
    if (status == 0 && !save_file(out_path, out.data, out.size)) {
        std::cerr << "Failed to write LAC file: " << out_path << "\n";
        status = 2;
    }
    if (status == 0)
        std::cout << (re ? "Recompressed " : cut ? "Cut " : "Joined ") << res.frames << " frames, " << (int)res.channels << " ch, " << (int)res.bit_depth << " bit, "
                  << res.sample_rate << " Hz: " << res.source_lac_bytes << " -> " << res.lac_bytes << " bytes, data_crc32=" << std::hex << res.data_crc32 << std::dec
                  << (res.verified ? ", verified" : "") << " -> " << out_path << "\n";
    if (out.data) lacx_free(const_cast<uint8_t*>(out.data));
    lacx_decoder_destroy(dec);
    lacx_encoder_destroy(enc);
    return status;
}

// "12.345": n / rate seconds, cut to milliseconds, in integers
std::string seconds_of(uint64_t n, uint32_t rate) {
    const unsigned __int128 ms = (unsigned __int128)n * 1000u / (rate ? rate : 1u);
    char text[48];
    std::snprintf(text, sizeof(text), "%llu.%03u", (unsigned long long)(ms / 1000u), (unsigned)(ms % 1000u));
    return text;
}

bool plain_number(const std::string& v, uint64_t& out) {
    if (v.empty() || v.size() > 18) return false;
    for (char c : v)
        if (c < '0' || c > '9') return false;
    out = std::stoull(v);
    return true;
}

// lacx_cli find FILE... : the runs of every .lac (what it decodes to, leniently: a lost block splits a run) and of every
// WAV's data chunk, found on the device (lacx_decoder_runs_batch_device / lacx_decoder_runs_pcm_batch_device), the files of
// each kind as one job.  A level in dBFS becomes floor(2^(b-1) * 10^(dB/20)) at each file's depth b, --clip is 2^(b-1)-1,
// seconds become frames at each file's rate.  Per file in argument order one line per run, then one totals line per
// detector.  Exit 0 nothing found, 1 runs found, 2 a file was refused (its message on stderr).
int find_command(int argc, char** argv) {
    struct Want {
        uint8_t kind;
        bool db, clip;
        double dbfs;
        uint64_t level;
    };
    std::vector<Want> wants;
    std::vector<const char*> paths;
    uint8_t channel = LACX_RUN_ALL;
    uint64_t min_frames = 1;
    double min_seconds = -1.0;
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        bool ok = true;
        Want w{LACX_RUN_QUIET, false, false, 0.0, 0};
        char* end = nullptr;
        if (a.compare(0, 2, "--") != 0) paths.push_back(argv[i]);
        else if (a.compare(0, 8, "--quiet=") == 0) ok = plain_number(a.substr(8), w.level) && w.level <= 0xFFFFFFFFull, wants.push_back(w);
        else if (a.compare(0, 11, "--quiet-db=") == 0) w.db = true, w.dbfs = std::strtod(a.c_str() + 11, &end), ok = end != a.c_str() + 11 && !*end, wants.push_back(w);
        else if (a.compare(0, 7, "--peak=") == 0) w.kind = LACX_RUN_PEAK, ok = plain_number(a.substr(7), w.level) && w.level <= 0xFFFFFFFFull, wants.push_back(w);
        else if (a == "--clip") w.kind = LACX_RUN_PEAK, w.clip = true, wants.push_back(w);
        else if (a == "--flat") w.kind = LACX_RUN_FLAT, wants.push_back(w);
        else if (a == "--channel=left") channel = 0;
        else if (a == "--channel=right") channel = 1;
        else if (a == "--channel=all") channel = LACX_RUN_ALL;
        else if (a.compare(0, 6, "--min=") == 0) ok = plain_number(a.substr(6), min_frames) && min_frames >= 1;
        else if (a.compare(0, 14, "--min-seconds=") == 0) min_seconds = std::strtod(a.c_str() + 14, &end), ok = end != a.c_str() + 14 && !*end && min_seconds >= 0.0;
        else ok = false;
        if (!ok) {
            usage();
            return 2;
        }
    }
    const int n = (int)paths.size();
    if (n == 0 || wants.empty() || wants.size() > LACX_MAX_DETECTORS) {
        usage();
        return 2;
    }
    const uint32_t nd = (uint32_t)wants.size();
    std::vector<std::vector<uint8_t>> data(n);
    std::vector<std::string> error(n);
    std::vector<lacx_runs_result> result(n, lacx_runs_result{});
    std::vector<std::vector<std::vector<lacx_run>>> lists(n);
    std::vector<lacx_run_detector> dets((size_t)n * nd);  // file i's detectors: dets[i * nd ...]
    std::vector<int> lacs, wavs;
    std::vector<lacx_wav_info> winfo(n, lacx_wav_info{});
    auto resolve = [&](int i, uint32_t bits, uint32_t rate) {
        for (uint32_t k = 0; k < nd; ++k) {
            const Want& w = wants[k];
            lacx_run_detector d{};
            d.kind = w.kind;
            d.channel = channel;
            const double full = (double)(1u << (bits - 1));
            d.level = w.clip ? (1u << (bits - 1)) - 1u : w.db ? (uint32_t)std::floor(std::min(full * std::pow(10.0, w.dbfs / 20.0), 4294967295.0)) : (uint32_t)w.level;
            d.min_frames = min_seconds >= 0.0 ? std::max<uint64_t>(1, (uint64_t)std::floor(min_seconds * rate)) : min_frames;
            dets[(size_t)i * nd + k] = d;
        }
    };
    for (int i = 0; i < n; ++i) {
        if (!load_file(paths[i], data[i])) {
            error[i] = "Failed to read file";
        } else if (data[i].size() >= 4 && std::memcmp(data[i].data(), "RIFF", 4) == 0) {
            if (lacx_wav_parse(data[i].data(), data[i].size(), &winfo[i]) != LACX_OK) error[i] = "Failed to read WAV";
            else wavs.push_back(i), resolve(i, winfo[i].bit_depth, winfo[i].sample_rate);
        } else {
            lacx_stream_info info{};
            uint32_t present = 0, flags = 0;
            if (lacx_stream_scan(data[i].data(), data[i].size(), &info, &present, &flags) != LACX_OK) error[i] = lacx_decode_last_error();
            else lacs.push_back(i), resolve(i, info.bit_depth, info.sample_rate);
        }
    }
    lacx_decoder* dec = nullptr;
    if (lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: lacx_decoder_create failed\n";
        return 2;
    }
    auto collect = [&](const std::vector<int>& which, int rc, const std::vector<int>& item_rc, const std::vector<lacx_runs_result>& out) {
        for (size_t k = 0; k < which.size(); ++k) {
            if (item_rc[k] != LACX_OK || rc == LACX_E_DEVICE) {
                error[which[k]] = rc == LACX_E_DEVICE || item_rc[k] == LACX_OK ? lacx_decode_last_error() : lacx_decoder_item_error(dec, (uint32_t)k);
                continue;
            }
            result[which[k]] = out[k];
            lists[which[k]].resize(nd);
            for (uint32_t q = 0; q < nd; ++q) {
                const lacx_run* r = nullptr;
                uint64_t count = 0;
                if (lacx_decoder_item_runs(dec, (uint32_t)k, q, &r, &count) == LACX_OK) lists[which[k]][q].assign(r, r + count);
            }
        }
    };
    auto queries_of = [&](const std::vector<int>& which) {
        std::vector<lacx_run_query> q;
        for (int i : which) q.push_back(lacx_run_query{(uint32_t)i * nd, nd});
        return q;
    };
    if (!lacs.empty()) {
        std::vector<lacx_span> spans;
        for (int i : lacs) spans.push_back(lacx_span{data[i].data(), data[i].size()});
        const std::vector<lacx_run_query> q = queries_of(lacs);
        std::vector<int> item_rc(lacs.size(), LACX_OK);
        std::vector<lacx_runs_result> out(lacs.size());
        const int rc = lacx_decoder_runs_batch_device(dec, spans.data(), q.data(), (uint32_t)spans.size(), dets.data(), (uint32_t)dets.size(), nullptr,
                                                      item_rc.data(), out.data(), nullptr);
        collect(lacs, rc, item_rc, out);
    }
    if (!wavs.empty()) {
        std::vector<lacx_digest_source> src;
        std::vector<void*> dev;
        std::vector<int> sent;
        for (int i : wavs) {
            const lacx_wav_info& w = winfo[i];
            const uint64_t bytes = w.frames * w.channels * (uint64_t)(w.bit_depth / 8);
            void* p = nullptr;
            if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess ||
                hipMemcpy(p, data[i].data() + w.data_offset, bytes, hipMemcpyHostToDevice) != hipSuccess) {
                error[i] = "Failed to upload WAV data to the device";
                if (p) (void)hipFree(p);
                continue;
            }
            lacx_digest_source s{};
            s.pcm = lacx_pcm{p, nullptr, w.bit_depth == 16 ? LACX_PCM_INTERLEAVED_I16 : LACX_PCM_INTERLEAVED_I24, w.channels};
            s.frames = w.frames;
            s.sample_rate = w.sample_rate;
            s.bit_depth = (uint8_t)w.bit_depth;
            src.push_back(s), dev.push_back(p), sent.push_back(i);
        }
        if (!src.empty()) {
            const std::vector<lacx_run_query> q = queries_of(sent);
            std::vector<int> item_rc(src.size(), LACX_OK);
            std::vector<lacx_runs_result> out(src.size());
            const int rc = lacx_decoder_runs_pcm_batch_device(dec, src.data(), q.data(), (uint32_t)src.size(), dets.data(), (uint32_t)dets.size(), nullptr,
                                                              item_rc.data(), out.data(), nullptr);
            collect(sent, rc, item_rc, out);
        }
        for (void* p : dev) (void)hipFree(p);
    }
    lacx_decoder_destroy(dec);
    static const char* const kNames[] = {"quiet", "peak", "flat"};
    bool refused = false, found = false;
    for (int i = 0; i < n; ++i) {
        if (!error[i].empty()) {
            std::cerr << "Find failed: " << paths[i] << ": " << error[i] << "\n";
            refused = true;
            continue;
        }
        const lacx_runs_result& t = result[i];
        for (uint32_t q = 0; q < nd; ++q) {
            const lacx_run_detector& d = dets[(size_t)i * nd + q];
            for (const lacx_run& r : lists[i][q]) {
                found = true;
                std::cout << kNames[d.kind] << " start=" << r.start << " frames=" << r.frames << " at=" << seconds_of(r.start, t.sample_rate)
                          << "s length=" << seconds_of(r.frames, t.sample_rate) << "s " << paths[i] << "\n";
            }
        }
        for (uint32_t q = 0; q < nd; ++q) {
            const lacx_run_detector& d = dets[(size_t)i * nd + q];
            const lacx_run_totals& s = t.det[q];
            std::cout << kNames[d.kind] << " total level=" << d.level << " min=" << d.min_frames << " runs=" << s.runs << " frames=" << s.frames
                      << " longest=" << s.longest << " longest_start=" << s.longest_start << " of=" << t.frames << " lost_blocks=" << t.lost_blocks << " "
                      << paths[i] << "\n";
        }
    }
    return refused ? 2 : found ? 1 : 0;
}

// lacx_cli split in.lac PREFIX --quiet=LEVEL --min=FRAMES [--pad=N] [--verify]: one QUIET detector over all channels, the
// sounding pieces between its runs widened by --pad frames, clipped to the stream and merged where they touch, then one
// lacx_transcode_batch with one output per piece: PREFIX0001.lac, ...  A stream with a lost block is refused (silence cannot
// be told from loss); one that is all silence writes nothing.  Exit 0 done, 1 mismatch under --verify, 2 refused.
int split_command(int argc, char** argv) {
    const std::string in_path = argv[2], prefix = argv[3];
    uint64_t level = 0, min_frames = 0, pad = 0;
    bool verify = false, have_level = false, have_min = false;
    for (int i = 4; i < argc; ++i) {
        const std::string a = argv[i];
        bool ok = a == "--verify";
        if (ok) verify = true;
        if (a.compare(0, 8, "--quiet=") == 0) ok = have_level = plain_number(a.substr(8), level) && level <= 0xFFFFFFFFull;
        if (a.compare(0, 6, "--min=") == 0) ok = have_min = plain_number(a.substr(6), min_frames) && min_frames >= 1;
        if (a.compare(0, 6, "--pad=") == 0) ok = plain_number(a.substr(6), pad);
        if (!ok) {
            usage();
            return 2;
        }
    }
    if (!have_level || !have_min) {
        usage();
        return 2;
    }
    std::vector<uint8_t> file;
    if (!load_file(in_path, file)) {
        std::cerr << "Failed to read LAC file: " << in_path << "\n";
        return 2;
    }
    lacx_config cfg{};
    cfg.sample_rate = 48000;  // (the outputs' formats come from their source)
    cfg.bit_depth = 16;
    cfg.zero_run_enabled = 1;
    cfg.partitioning_enabled = 1;
    cfg.device = -1;
    lacx_encoder* enc = nullptr;
    lacx_decoder* dec = nullptr;
    if (lacx_encoder_create(&cfg, &enc) != LACX_OK || lacx_decoder_create(-1, &dec) != LACX_OK) {
        std::cerr << "Error: cannot create the encoder and the decoder\n";
        if (enc) lacx_encoder_destroy(enc);
        return 2;
    }
    auto done = [&](int status) {
        lacx_decoder_destroy(dec);
        lacx_encoder_destroy(enc);
        return status;
    };
    lacx_run_detector det{};
    det.kind = LACX_RUN_QUIET, det.channel = LACX_RUN_ALL, det.level = (uint32_t)level, det.min_frames = min_frames;
    const lacx_span span{file.data(), file.size()};
    const lacx_run_query query{0, 1};
    lacx_runs_result res{};
    if (lacx_decoder_runs_batch_device(dec, &span, &query, 1, &det, 1, nullptr, nullptr, &res, nullptr) != LACX_OK) {
        std::cerr << "Refused: " << lacx_decode_last_error() << "\n";
        return done(2);
    }
    if (res.lost_blocks) {
        std::cerr << "Refused: " << res.lost_blocks << " lost blocks: silence cannot be told from loss\n";
        return done(2);
    }
    const lacx_run* runs = nullptr;
    uint64_t count = 0;
    (void)lacx_decoder_item_runs(dec, 0, 0, &runs, &count);
    std::vector<lacx_run> pieces;  // [start, start + frames)
    uint64_t at = 0;
    for (uint64_t k = 0; k <= count; ++k) {
        const uint64_t start = k < count ? runs[k].start : res.frames, n = k < count ? runs[k].frames : 0;
        if (start > at) {
            const uint64_t lo = at > pad ? at - pad : 0, hi = res.frames - start > pad ? start + pad : res.frames;
            if (!pieces.empty() && lo <= pieces.back().start + pieces.back().frames) pieces.back().frames = std::max(pieces.back().start + pieces.back().frames, hi) - pieces.back().start;
            else pieces.push_back(lacx_run{lo, hi - lo});
        }
        at = std::max(at, start + n);
    }
    if (pieces.empty()) {
        std::cout << "Split " << in_path << ": all " << res.frames << " frames are silence, nothing written\n";
        return done(0);
    }
    std::vector<lacx_edit_segment> segs;
    std::vector<lacx_edit_output> outs;
    for (const lacx_run& p : pieces) {
        lacx_edit_output o{};
        o.stereo_mode = 2;
        o.first_segment = (uint32_t)segs.size();
        o.segments = 1;
        outs.push_back(o);
        segs.push_back(lacx_edit_segment{file.data(), file.size(), p.start, p.frames});
    }
    std::vector<lacx_span> spans(outs.size(), lacx_span{});
    std::vector<lacx_edit_result> er(outs.size(), lacx_edit_result{});
    const int rc = lacx_transcode_batch(dec, enc, segs.data(), (uint32_t)segs.size(), outs.data(), (uint32_t)outs.size(), verify ? LACX_TRANSCODE_VERIFY : 0u,
                                        spans.data(), nullptr, er.data(), nullptr);
    int status = rc == LACX_OK ? 0 : rc == LACX_E_MISMATCH ? 1 : 2;
    if (status == 2) std::cerr << (rc == LACX_E_INVALID ? "Refused: " : "Error: ") << lacx_decode_last_error() << "\n";
    if (status == 1) std::cerr << "Verify failed: " << lacx_decode_last_error() << "\n";
    for (size_t k = 0; status == 0 && k < pieces.size(); ++k) {
        char number[24];
        std::snprintf(number, sizeof(number), "%04zu", k + 1);
        const std::string path = prefix + number + ".lac";
        if (!save_file(path, spans[k].data, spans[k].size)) {
            std::cerr << "Failed to write LAC file: " << path << "\n";
            status = 2;
            break;
        }
        std::cout << "Piece " << (k + 1) << " start=" << pieces[k].start << " frames=" << pieces[k].frames << " data_crc32=" << std::hex << er[k].data_crc32 << std::dec
                  << (er[k].verified ? ", verified" : "") << " -> " << path << "\n";
    }
    for (const lacx_span& s : spans)
        if (s.data) lacx_free(const_cast<uint8_t*>(s.data));
    return done(status);
}

struct Encoded {
    const uint8_t* data = nullptr;
    uint64_t size = 0;
};

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "selftest" && argc == 2) return selftest_command();
    if (mode == "verify" && argc == 4) return verify_command(argv);
    if (mode == "digest" && argc >= 3) return digest_command(argc, argv);
    if (mode == "stats" && argc >= 3) return stats_command(argc, argv);
    if (mode == "loudness") return loudness_command(argc, argv);
    if (mode == "peak") return peak_command(argc, argv);
    if (mode == "spectrum") return spectrum_command(argc, argv);
    if (mode == "accuraterip") return accuraterip_command(argc, argv);
    if (mode == "compare") return compare_command(argc, argv);
    if (mode == "inspect" && argc >= 3) return inspect_command(argc, argv);
    if (mode == "find" && argc >= 3) return find_command(argc, argv);
    if (mode == "split" && argc >= 4) return split_command(argc, argv);
    if (mode == "manifest" && argc == 4) return manifest_command(argv);
    if (mode == "check" && argc == 4) return check_command(argv);
    if (mode == "protect" && argc >= 4) return protect_command(argc, argv);
    if (mode == "repair" && argc >= 5) return repair_command(argc, argv);
    if ((mode == "recompress" || mode == "cut" || mode == "join") && argc >= 4) return transcode_command(mode, argc, argv);
    if (argc < 4 || (mode != "encode" && mode != "decode")) {
        usage();
        return 1;
    }
    if (mode == "decode") return decode_command(argc, argv);
    const std::string in_path = argv[2], out_path = argv[3];
    if (same_file(in_path, out_path)) {
        std::cerr << "Input and output paths must be different\n";
        return 1;
    }
    uint8_t stereo_mode = 2;
    bool partitioning = true, debug_threads = false, debug_zr = false, verify = false;
    unsigned long long threads = 0;
    std::string verify_path;  // --verify-against: another copy of the source (the master the input was made from)
    std::string manifest_path;  // --manifest: the manifest of what the written stream decodes to
    std::string recovery_path;  // --recovery: the recovery sidecar of the written bytes (default parameters)
    for (int i = 4; i < argc; ++i) {
        const std::string flag = argv[i];
        const std::string tprefix = "--threads=", vprefix = "--verify-against=", mprefix = "--manifest=", rprefix = "--recovery=";
        if (flag.compare(0, mprefix.size(), mprefix) == 0 && flag.size() > mprefix.size()) {
            manifest_path = flag.substr(mprefix.size());
        } else if (flag.compare(0, rprefix.size(), rprefix) == 0 && flag.size() > rprefix.size()) {
            recovery_path = flag.substr(rprefix.size());
        } else if (flag == "--no-partitioning") {
            partitioning = false;
        } else if (flag == "--stereo-mode=lr") {
            stereo_mode = 0;
        } else if (flag == "--stereo-mode=ms") {
            stereo_mode = 1;
        } else if (flag == "--debug-threads") {
            debug_threads = true;
        } else if (flag == "--debug-zr") {
            debug_zr = true;
        } else if (flag == "--verify") {
            verify = true;
        } else if (flag.compare(0, vprefix.size(), vprefix) == 0 && flag.size() > vprefix.size()) {
            verify = true;
            verify_path = flag.substr(vprefix.size());
        } else if (flag == "--debug-lpc" || flag == "--debug-stereo-est" || flag == "--debug-partitions") {
            // accepted like the reference does; its per-block log lines only exist in debug builds (LAC_DEBUG_LOG)
        } else if (flag.compare(0, tprefix.size(), tprefix) == 0) {
            if (!positive_integer(flag.substr(tprefix.size()), threads)) {
                std::cerr << "Error: --threads requires a positive integer\n";
                return 1;
            }
        } else {
            usage();
            return 1;
        }
    }
    if (!resolve_threads(threads)) return 1;
    std::ifstream in(in_path, std::ios::binary);
    std::vector<uint8_t> wav;
    if (in) wav.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    lacx_wav_info info{};
    if (!in || lacx_wav_parse(wav.data(), wav.size(), &info) != LACX_OK) {
        std::cerr << "Failed to read WAV: " << in_path << "\n";
        return 1;
    }
    lacx_config cfg{};
    cfg.sample_rate = info.sample_rate;
    cfg.bit_depth = (uint8_t)info.bit_depth;
    cfg.stereo_mode = info.channels == 1 ? 0 : stereo_mode;
    cfg.zero_run_enabled = 1;
    cfg.partitioning_enabled = partitioning ? 1 : 0;
    cfg.device = LACX_DEVICE_ALL;  // every visible device: the blocks fan out over them (the reference spreads them over its threads)
    cfg.emit_threads = (uint32_t)(threads > 0xFFFFFFFFull ? 0xFFFFFFFFull : threads);
    lacx_encoder* enc = nullptr;
    if (lacx_encoder_create(&cfg, &enc) != LACX_OK) {
        std::cerr << "Error: lacx_encoder_create failed\n";
        return 1;
    }
    Encoded lac;
    if (lacx_encode_wav_view(enc, wav.data(), wav.size(), &lac.data, &lac.size) != LACX_OK) {
        std::cerr << "Error: " << lacx_last_error(enc) << "\n";
        lacx_encoder_destroy(enc);
        return 1;
    }
    if (debug_zr) {  // the same stream without the zero-run mode, for the gain line (ref src/main.cpp:677-689)
        lacx_config base_cfg = cfg;
        base_cfg.zero_run_enabled = 0;
        lacx_encoder* base = nullptr;
        Encoded b;
        if (lacx_encoder_create(&base_cfg, &base) != LACX_OK ||
            lacx_encode_wav_view(base, wav.data(), wav.size(), &b.data, &b.size) != LACX_OK) {
            std::cerr << "Error: " << (base ? lacx_last_error(base) : "lacx_encoder_create failed") << "\n";
            if (base) lacx_encoder_destroy(base);
            lacx_encoder_destroy(enc);
            return 1;
        }
        const double gain = b.size ? (1.0 - (double)lac.size / (double)b.size) * 100.0 : 0.0;
        std::cout << "[debug-zr] baseline_bytes=" << b.size << " zr_bytes=" << lac.size << " gain=" << gain << "%\n";
        lacx_encoder_destroy(base);
    }
    if (verify) {  // the produced bytes against the input file image, on the device, before anything is published
        std::vector<uint8_t> other;
        if (!verify_path.empty() && !load_file(verify_path, other)) {
            std::cerr << "Failed to read WAV: " << verify_path << "\n";
            lacx_encoder_destroy(enc);
            return 1;
        }
        const std::vector<uint8_t>& against = verify_path.empty() ? wav : other;
        lacx_decoder* dec = nullptr;
        lacx_verify_result res{};
        int vrc = lacx_decoder_create(-1, &dec);
        if (vrc == LACX_OK) vrc = lacx_decoder_verify_wav(dec, lac.data, lac.size, against.data(), against.size(), &res, nullptr);
        if (vrc != LACX_OK) {
            std::cerr << "Verify failed: " << (dec ? lacx_decode_last_error() : "lacx_decoder_create failed") << "\n";
            if (dec) lacx_decoder_destroy(dec);
            lacx_encoder_destroy(enc);
            return 1;
        }
        lacx_decoder_destroy(dec);
    }
    if (!manifest_path.empty()) {  // of the produced bytes, before anything is published; with --verify: the source's own
        std::vector<uint8_t> m;
        std::string err;
        if (same_file(manifest_path, out_path) || same_file(manifest_path, in_path)) err = "the manifest needs a path of its own";
        if (!err.empty() || !make_manifest(lac.data, lac.size, m, err) || !save_file(manifest_path, m.data(), m.size())) {
            std::cerr << "Manifest failed: " << (err.empty() ? "cannot write " + manifest_path : err) << "\n";
            lacx_encoder_destroy(enc);
            return 1;
        }
    }
    if (!recovery_path.empty()) {  // of the produced bytes, before anything is published
        std::vector<uint8_t> m;
        std::string err;
        if (same_file(recovery_path, out_path) || same_file(recovery_path, in_path) || (!manifest_path.empty() && same_file(recovery_path, manifest_path)))
            err = "the recovery data needs a path of its own";
        if (!err.empty() || !make_recovery(lac.data, lac.size, lacx_recovery_params{}, m, err) || !save_file(recovery_path, m.data(), m.size())) {
            std::cerr << "Recovery data failed: " << (err.empty() ? "cannot write " + recovery_path : err) << "\n";
            lacx_encoder_destroy(enc);
            return 1;
        }
    }
    const std::string tmp = out_path + ".lacx-partial";
    bool ok = false;
    {
        std::ofstream out(tmp, std::ios::binary | std::ios::trunc);
        ok = out && out.write(reinterpret_cast<const char*>(lac.data), (std::streamsize)lac.size) && out.flush();
    }
    ok = ok && !same_file(in_path, out_path) && std::rename(tmp.c_str(), out_path.c_str()) == 0;
    const uint64_t size = lac.size;
    lacx_encoder_destroy(enc);  // the view dies with the encoder
    if (!ok) {
        std::remove(tmp.c_str());
        std::cerr << "Failed to write LAC file: " << out_path << "\n";
        return 1;
    }
    std::cout << "Encoded " << in_path << " -> " << out_path << " (" << size << " bytes)\n";
    if (debug_threads) {
        // The block loop runs on the device; on the host the encode call uses the calling thread (the emit pool only
        // exists with LACX_FLAG_HOST_EMIT), which is what the reference reports for a one-thread run (ref :699-709).
        std::cout << "Thread usage: 1 threads\n  " << std::this_thread::get_id() << "\n";
        std::cout << "WARNING: Multi-threading not active (single-threaded execution).\n";
    }
    return 0;
}
