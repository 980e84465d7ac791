"""ctypes binding of liblacx.so (include/lacx.h) and Python mirrors of the reference's encoder classes.

`Encoder` mirrors LAC::Encoder (ref src/codec/lac/encoder.hpp:12-43): same constructor argument
order, the same setters, `encode(left, right)` returning the .lac bytes, ValueError where the
reference throws std::invalid_argument and RuntimeError where it throws std::runtime_error.
`BlockEncoder` mirrors Block::Encoder (ref src/codec/block/encoder.hpp:9-30).

PyTorch is optional plumbing: `encode_tensors` takes int32 CUDA(HIP) tensors whose storage is handed
to the library by raw pointer (no torch types cross the ABI).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liblacx.so")
# the diagnostic twin (analysis kernel built with -DLACX_TEST_HOOKS: honours LACX_DEBUG_SKIP); tests and timing
# experiments select it explicitly with use_library(HOOKS_LIB_PATH) -- the product never loads it by itself
HOOKS_LIB_PATH = os.path.join(HERE, "liblacx_hooks.so")
DEVICE_ALL = -2
MAX_FANOUT = 16

OK, E_INVALID, E_RUNTIME, E_DEVICE, E_MISMATCH = 0, 1, 2, 3, 4
MAX_BLOCK = 16384
SLOTS = 16
CH_L, CH_R, CH_M, CH_S = 0, 1, 2, 3


class Config(C.Structure):
    _fields_ = [
        ("sample_rate", C.c_uint32),
        ("bit_depth", C.c_uint8),
        ("stereo_mode", C.c_uint8),
        ("zero_run_enabled", C.c_uint8),
        ("partitioning_enabled", C.c_uint8),
        ("device", C.c_int32),
        ("emit_threads", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class ChannelPlan(C.Structure):
    _fields_ = [
        ("predictor_type", C.c_uint8),
        ("order", C.c_uint8),
        ("partition_order", C.c_uint8),
        ("valid", C.c_uint8),
        ("coef", C.c_int16 * 12),
        ("payload_bytes", C.c_uint32),
        ("total_bits", C.c_uint64),
        ("part_mode_k", C.c_uint8 * 256),
    ]


class BlockPlan(C.Structure):
    _fields_ = [
        ("choose_ms", C.c_uint8),
        ("uncertain", C.c_uint8),
        ("est_ms", C.c_uint8),
        ("invalid", C.c_uint8),
        ("frames", C.c_uint32),
        ("first_bad", C.c_uint32),
        ("pad", C.c_uint32),
    ]


class Timing(C.Structure):
    _fields_ = [
        ("h2d_ms", C.c_double),
        ("analysis_ms", C.c_double),
        ("ingest_ms", C.c_double),
        ("probe_ms", C.c_double),
        ("full_ms", C.c_double),
        ("d2h_ms", C.c_double),
        ("emit_ms", C.c_double),
        ("total_ms", C.c_double),
        ("full_slots", C.c_uint64),
        ("probe_slots", C.c_uint64),
        ("full_launches", C.c_uint32),
        ("regrows", C.c_uint32),
        ("full_exec_ms", C.c_double),
        ("emit_direct", C.c_uint32),
        ("moved_by_k_pack", C.c_uint32),
        ("packer_gave_up", C.c_uint32),
        ("drain_copies", C.c_uint32),
        ("drain_first_ms", C.c_double),
        ("drain_last_ms", C.c_double),
        ("poll_gap_max_ms", C.c_double),
        ("kernels_done_ms", C.c_double),
        ("enqueue_ms", C.c_double),
        ("silent_copies", C.c_uint32),
        ("reserved0", C.c_uint32),
    ]


EXPORTS = (
    "lacx_encoder_create", "lacx_encoder_destroy", "lacx_last_error", "lacx_free", "lacx_get_timing",
    "lacx_encode", "lacx_encode_device", "lacx_analyze", "lacx_analyze_device", "lacx_emit_from_plans",
    "lacx_encode_shard", "lacx_encode_shard_device", "lacx_encode_shard_device_view", "lacx_encode_shard_pcm_device_view", "lacx_assemble", "lacx_block_encode",
    "lacx_block_plan_only", "lacx_debug_lpc", "lacx_debug_stamps", "lacx_device_count", "lacx_wav_parse",
    "lacx_encode_wav", "lacx_encode_shard_pcm_device_begin", "lacx_encode_shard_end", "lacx_debug_emit_workers", "lacx_encode_wav_view",
    "lacx_stream_parse", "lacx_decode", "lacx_decode_last_error", "lacx_encode_batch_device",
    "lacx_encoder_create_multi", "lacx_encoder_lanes", "lacx_fanout_range", "lacx_encode_fanout_resident",
    "lacx_get_fanout_stats", "lacx_get_lane_timing", "lacx_fanout_exchange_note",
    "lacx_decoder_create", "lacx_decoder_destroy", "lacx_decoder_decode", "lacx_sizeof",
    "lacx_decoder_decode_wav", "lacx_decoder_decode_wav_view",
    "lacx_decoder_decode_wav_batch", "lacx_decoder_decode_wav_batch_view", "lacx_decoder_decode_batch_device",
    "lacx_decoder_item_error", "lacx_decoder_decode_window_batch_device", "lacx_decoder_decode_window",
    "lacx_decoder_verify_batch_device", "lacx_decoder_verify_wav",
    "lacx_decoder_digest_batch_device", "lacx_decoder_digest_pcm_batch_device", "lacx_crc32_combine",
    "lacx_stream_scan", "lacx_decoder_salvage_wav_batch_view", "lacx_decoder_salvage_wav",
    "lacx_decoder_salvage_batch_device", "lacx_decoder_item_faults", "lacx_block_fault_text",
    "lacx_decoder_digest_blocks_batch_device", "lacx_decoder_item_block_digests", "lacx_decoder_digest_pcm_blocks_batch_device",
    "lacx_manifest_build", "lacx_manifest_parse", "lacx_decoder_check_batch_device",
    "lacx_decoder_salvage_wav_batch_view_checked", "lacx_decoder_salvage_batch_device_checked",
    "lacx_recovery_build_batch_view", "lacx_recovery_build", "lacx_recovery_parse", "lacx_recovery_scan_batch",
    "lacx_recovery_repair_batch_view", "lacx_recovery_repair", "lacx_decoder_item_bad_slices",
    "lacx_decoder_stats_batch_device", "lacx_decoder_stats_pcm_batch_device", "lacx_decoder_item_block_stats", "lacx_stats_combine",
    "lacx_decoder_loudness_batch_device", "lacx_decoder_loudness_pcm_batch_device", "lacx_decoder_item_loudness_rows", "lacx_loudness_combine",
    "lacx_decoder_truepeak_batch_device", "lacx_decoder_truepeak_pcm_batch_device", "lacx_decoder_item_truepeak_rows", "lacx_truepeak_combine",
    "lacx_decoder_spectrum_batch_device", "lacx_decoder_spectrum_pcm_batch_device", "lacx_decoder_item_spectrum_rows", "lacx_spectrum_combine",
    "lacx_decoder_accuraterip_batch_device", "lacx_decoder_accuraterip_pcm_batch_device", "lacx_decoder_item_ar_tracks", "lacx_decoder_item_ar_sums",
    "lacx_ar_ids",
    "lacx_decoder_compare_batch_device", "lacx_decoder_compare_pcm_batch_device", "lacx_decoder_item_compare_rows", "lacx_decoder_item_compare_counts",
    "lacx_compare_combine",
    "lacx_decoder_inspect_batch_device", "lacx_decoder_item_block_info", "lacx_decoder_item_partitions", "lacx_inspect_combine",
    "lacx_decoder_inspect_guard", "lacx_transcode_batch",
    "lacx_decoder_runs_batch_device", "lacx_decoder_runs_pcm_batch_device", "lacx_decoder_item_runs",
)


def build(force: bool = False) -> str:
    """Compiles liblacx.so in-tree (hipcc cross-compiles gfx950 without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", HERE, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", HERE, "liblacx.so", "liblacx_hooks.so"], stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None
_lib_path = LIB_PATH
_libs = {}


def use_library(path: str | None = None):
    """Selects the shared library the binding calls from now on (None: the product's liblacx.so).  For the parity tests
    that need the hooks build and for A/B experiments of differently built libraries (scripts/kexp.py); encoders created
    before the switch must not be used after it."""
    global _lib, _lib_path
    _lib_path = path or LIB_PATH
    _lib = None


def lib():
    global _lib
    if _lib is None:
        path = _lib_path
        if path in _libs:
            _lib = _libs[path]
            return _lib
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: build it with `make -C {HERE}` (or __graft_entry__.build()); "
                "the LAC encode path has no Python/CPU fallback")
        L = C.CDLL(path)
        L.lacx_last_error.restype = C.c_char_p
        L.lacx_last_error.argtypes = [C.c_void_p]
        L.lacx_free.argtypes = [C.c_void_p]
        L.lacx_encoder_destroy.argtypes = [C.c_void_p]
        L.lacx_get_timing.argtypes = [C.c_void_p, C.POINTER(Timing)]
        L.lacx_device_count.restype = C.c_int
        L.lacx_decode_last_error.restype = C.c_char_p
        L.lacx_fanout_exchange_note.restype = C.c_char_p
        L.lacx_fanout_exchange_note.argtypes = [C.c_void_p]
        L.lacx_encoder_lanes.restype = C.c_uint32
        L.lacx_encoder_lanes.argtypes = [C.c_void_p]
        L.lacx_fanout_range.restype = None
        L.lacx_decoder_decode_wav.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.POINTER(C.c_uint8)),
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
        L.lacx_decoder_decode_wav_view.argtypes = L.lacx_decoder_decode_wav.argtypes
        L.lacx_decoder_decode_wav_batch_view.argtypes = [C.c_void_p, C.POINTER(Span), C.c_uint32, C.POINTER(Span),
                                                         C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.lacx_decoder_decode_wav_batch.argtypes = L.lacx_decoder_decode_wav_batch_view.argtypes
        L.lacx_decoder_decode_batch_device.argtypes = [C.c_void_p, C.POINTER(DecodeItem), C.c_uint32, C.c_void_p,
                                                       C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.lacx_decoder_decode_window_batch_device.argtypes = [C.c_void_p, C.POINTER(WindowItem), C.c_uint32, C.c_int,
                                                              C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.lacx_decoder_decode_window.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.lacx_decoder_verify_batch_device.argtypes = [C.c_void_p, C.POINTER(VerifyItem), C.c_uint32, C.c_void_p,
                                                       C.POINTER(C.c_int), C.POINTER(VerifyResult), C.POINTER(C.c_float)]
        L.lacx_decoder_verify_wav.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint8), C.c_uint64,
                                              C.POINTER(VerifyResult), C.POINTER(C.c_float)]
        L.lacx_decoder_digest_batch_device.argtypes = [C.c_void_p, C.POINTER(Span), C.c_uint32, C.c_void_p, C.POINTER(C.c_int),
                                                       C.POINTER(Digest), C.POINTER(C.c_float)]
        L.lacx_decoder_digest_pcm_batch_device.argtypes = [C.c_void_p, C.POINTER(DigestSource), C.c_uint32, C.c_void_p,
                                                           C.POINTER(C.c_int), C.POINTER(Digest), C.POINTER(C.c_float)]
        L.lacx_crc32_combine.restype = C.c_uint32
        L.lacx_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
        L.lacx_stream_scan.argtypes = [C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(StreamInfo), C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint32)]
        L.lacx_decoder_salvage_wav_batch_view.argtypes = [C.c_void_p, C.POINTER(Span), C.c_uint32, C.POINTER(Span),
                                                          C.POINTER(C.c_int), C.POINTER(SalvageResult), C.POINTER(C.c_float)]
        L.lacx_decoder_salvage_wav.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.POINTER(C.c_uint8)),
                                               C.POINTER(C.c_uint64), C.POINTER(SalvageResult), C.POINTER(C.c_float)]
        L.lacx_decoder_salvage_batch_device.argtypes = [C.c_void_p, C.POINTER(DecodeItem), C.c_uint32, C.c_void_p,
                                                        C.POINTER(C.c_int), C.POINTER(SalvageResult), C.POINTER(C.c_float)]
        L.lacx_decoder_item_faults.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(BlockFault)), C.POINTER(C.c_uint32)]
        L.lacx_decoder_digest_blocks_batch_device.argtypes = L.lacx_decoder_digest_batch_device.argtypes
        L.lacx_decoder_item_block_digests.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(BlockDigest)), C.POINTER(C.c_uint32)]
        L.lacx_decoder_digest_pcm_blocks_batch_device.argtypes = [C.c_void_p, C.POINTER(DigestSource), C.c_uint32, C.c_uint32, C.c_void_p,
                                                                  C.POINTER(C.c_int), C.POINTER(Digest), C.POINTER(C.c_float)]
        L.lacx_manifest_build.argtypes = [C.POINTER(Digest), C.POINTER(BlockDigest), C.c_uint32, C.POINTER(C.POINTER(C.c_uint8)),
                                          C.POINTER(C.c_uint64)]
        L.lacx_manifest_parse.argtypes = [C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(ManifestInfo), C.POINTER(BlockDigest), C.c_uint32]
        L.lacx_decoder_check_batch_device.argtypes = [C.c_void_p, C.POINTER(Span), C.POINTER(Span), C.c_uint32, C.c_void_p,
                                                      C.POINTER(C.c_int), C.POINTER(SalvageResult), C.POINTER(C.c_float)]
        L.lacx_decoder_salvage_wav_batch_view_checked.argtypes = [C.c_void_p, C.POINTER(Span), C.POINTER(Span), C.c_uint32, C.POINTER(Span),
                                                                  C.POINTER(C.c_int), C.POINTER(SalvageResult), C.POINTER(C.c_float)]
        L.lacx_decoder_salvage_batch_device_checked.argtypes = [C.c_void_p, C.POINTER(DecodeItem), C.POINTER(Span), C.c_uint32, C.c_void_p,
                                                                C.POINTER(C.c_int), C.POINTER(SalvageResult), C.POINTER(C.c_float)]
        u8p = C.POINTER(C.c_uint8)
        L.lacx_recovery_build_batch_view.argtypes = [C.c_void_p, C.POINTER(Span), C.c_uint32, C.POINTER(RecoveryParams), C.POINTER(Span),
                                                     C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.lacx_recovery_build.argtypes = [C.c_void_p, u8p, C.c_uint64, C.POINTER(RecoveryParams), C.POINTER(u8p), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_float)]
        L.lacx_recovery_parse.argtypes = [u8p, C.c_uint64, C.POINTER(RecoveryInfo)]
        L.lacx_recovery_scan_batch.argtypes = [C.c_void_p, C.POINTER(Span), C.POINTER(Span), C.c_uint32, C.POINTER(C.c_int),
                                               C.POINTER(RepairResult), C.POINTER(C.c_float)]
        L.lacx_recovery_repair_batch_view.argtypes = [C.c_void_p, C.POINTER(Span), C.POINTER(Span), C.c_uint32, C.c_uint32, C.POINTER(Span),
                                                      C.POINTER(C.c_int), C.POINTER(RepairResult), C.POINTER(C.c_float)]
        L.lacx_recovery_repair.argtypes = [C.c_void_p, u8p, C.c_uint64, u8p, C.c_uint64, C.c_uint32, C.POINTER(u8p), C.POINTER(C.c_uint64),
                                           C.POINTER(RepairResult), C.POINTER(C.c_float)]
        L.lacx_decoder_item_bad_slices.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32)]
        L.lacx_decoder_stats_batch_device.argtypes = [C.c_void_p, C.POINTER(Span), C.c_uint32, C.c_void_p, C.POINTER(C.c_int),
                                                      C.POINTER(Stats), C.POINTER(C.c_float)]
        L.lacx_decoder_stats_pcm_batch_device.argtypes = [C.c_void_p, C.POINTER(DigestSource), C.c_uint32, C.c_uint32, C.c_void_p,
                                                          C.POINTER(C.c_int), C.POINTER(Stats), C.POINTER(C.c_float)]
        L.lacx_decoder_item_block_stats.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(BlockStats)), C.POINTER(C.c_uint32)]
        L.lacx_stats_combine.argtypes = [C.POINTER(BlockStats), C.c_uint32, C.c_uint8, C.c_uint8, C.c_uint32, C.POINTER(Stats)]
        L.lacx_decoder_loudness_batch_device.argtypes = [C.c_void_p, C.POINTER(Span), C.c_uint32, C.c_void_p, C.POINTER(C.c_int),
                                                         C.POINTER(Loudness), C.POINTER(C.c_float)]
        L.lacx_decoder_loudness_pcm_batch_device.argtypes = [C.c_void_p, C.POINTER(DigestSource), C.c_uint32, C.c_void_p, C.POINTER(C.c_int),
                                                             C.POINTER(Loudness), C.POINTER(C.c_float)]
        L.lacx_decoder_item_loudness_rows.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(LoudnessRow)), C.POINTER(C.c_uint32)]
        L.lacx_loudness_combine.argtypes = [C.POINTER(C.POINTER(LoudnessRow)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8),
                                            C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(Loudness)]
        L.lacx_decoder_truepeak_batch_device.argtypes = [C.c_void_p, C.POINTER(Span), C.c_uint32, C.c_void_p, C.POINTER(C.c_int),
                                                         C.POINTER(TruePeak), C.POINTER(C.c_float)]
        L.lacx_decoder_truepeak_pcm_batch_device.argtypes = [C.c_void_p, C.POINTER(DigestSource), C.c_uint32, C.c_void_p, C.POINTER(C.c_int),
                                                             C.POINTER(TruePeak), C.POINTER(C.c_float)]
        L.lacx_decoder_item_truepeak_rows.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(TruePeakRow)), C.POINTER(C.c_uint32)]
        L.lacx_truepeak_combine.argtypes = [C.POINTER(C.POINTER(TruePeakRow)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(TruePeak)]
        L.lacx_decoder_spectrum_batch_device.argtypes = [C.c_void_p, C.POINTER(Span), C.c_uint32, C.c_uint32, C.c_double, C.c_void_p, C.POINTER(C.c_int),
                                                         C.POINTER(Spectrum), C.POINTER(C.c_float)]
        L.lacx_decoder_spectrum_pcm_batch_device.argtypes = [C.c_void_p, C.POINTER(DigestSource), C.c_uint32, C.c_uint32, C.c_double, C.c_void_p,
                                                             C.POINTER(C.c_int), C.POINTER(Spectrum), C.POINTER(C.c_float)]
        L.lacx_decoder_item_spectrum_rows.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(SpectrumRow)), C.POINTER(C.c_uint32)]
        L.lacx_spectrum_combine.argtypes = [C.POINTER(SpectrumRow), C.c_uint32, C.c_uint8, C.c_uint8, C.c_uint64, C.c_uint32, C.c_uint32, C.c_double,
                                            C.POINTER(Spectrum)]
        u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        L.lacx_decoder_accuraterip_batch_device.argtypes = [C.c_void_p, C.POINTER(Span), C.c_uint32, u64p, C.c_uint32, C.POINTER(ArDisc), C.c_uint32,
                                                            C.c_void_p, C.POINTER(C.c_int), C.POINTER(ArResult), C.POINTER(C.c_float)]
        L.lacx_decoder_accuraterip_pcm_batch_device.argtypes = [C.c_void_p, C.POINTER(DigestSource), C.c_uint32, u64p, C.c_uint32, C.POINTER(ArDisc),
                                                                C.c_uint32, C.c_void_p, C.POINTER(C.c_int), C.POINTER(ArResult), C.POINTER(C.c_float)]
        L.lacx_decoder_item_ar_tracks.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(ArTrack)), u32p]
        L.lacx_decoder_item_ar_sums.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(u32p), C.POINTER(u32p), C.POINTER(u32p), u32p]
        L.lacx_ar_ids.argtypes = [u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ArId)]
        L.lacx_decoder_compare_batch_device.argtypes = [C.c_void_p, C.POINTER(Span), C.c_uint32, C.POINTER(ComparePair), C.c_uint32, C.c_void_p,
                                                        C.POINTER(C.c_int), C.POINTER(Compare), C.POINTER(C.c_float)]
        L.lacx_decoder_compare_pcm_batch_device.argtypes = [C.c_void_p, C.POINTER(DigestSource), C.c_uint32, C.POINTER(ComparePair), C.c_uint32, C.c_void_p,
                                                            C.POINTER(C.c_int), C.POINTER(Compare), C.POINTER(C.c_float)]
        L.lacx_decoder_item_compare_rows.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(CompareRow)), u32p]
        L.lacx_decoder_item_compare_counts.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(u64p), u32p]
        L.lacx_compare_combine.argtypes = [C.POINTER(CompareRow), C.c_uint32, C.c_uint8, C.c_uint8, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int64,
                                           C.POINTER(Compare)]
        L.lacx_decoder_inspect_batch_device.argtypes = [C.c_void_p, C.POINTER(Span), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_int),
                                                        C.POINTER(StreamReport), C.POINTER(C.c_float)]
        L.lacx_decoder_item_block_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(BlockInfo)), C.POINTER(C.c_uint32)]
        L.lacx_decoder_item_partitions.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(u8p),
                                                   C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32)]
        L.lacx_decoder_inspect_guard.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.lacx_inspect_combine.argtypes = [C.POINTER(BlockInfo), C.c_uint32, C.POINTER(StreamInfo), C.POINTER(StreamReport)]
        L.lacx_transcode_batch.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(EditSegment), C.c_uint32, C.POINTER(EditOutput), C.c_uint32,
                                           C.c_uint32, C.POINTER(Span), C.POINTER(C.c_int), C.POINTER(EditResult), C.POINTER(C.c_float)]
        L.lacx_decoder_runs_batch_device.argtypes = [C.c_void_p, C.POINTER(Span), C.POINTER(RunQuery), C.c_uint32, C.POINTER(RunDetector),
                                                     C.c_uint32, C.c_void_p, C.POINTER(C.c_int), C.POINTER(RunsResult), C.POINTER(C.c_float)]
        L.lacx_decoder_runs_pcm_batch_device.argtypes = [C.c_void_p, C.POINTER(DigestSource), C.POINTER(RunQuery), C.c_uint32,
                                                         C.POINTER(RunDetector), C.c_uint32, C.c_void_p, C.POINTER(C.c_int),
                                                         C.POINTER(RunsResult), C.POINTER(C.c_float)]
        L.lacx_decoder_item_runs.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.POINTER(Run)), C.POINTER(C.c_uint64)]
        L.lacx_block_fault_text.restype = C.c_char_p
        L.lacx_block_fault_text.argtypes = [C.c_uint32]
        L.lacx_decoder_item_error.restype = C.c_char_p
        L.lacx_decoder_item_error.argtypes = [C.c_void_p, C.c_uint32]
        # the structs declared in this file against the library's own sizeof(): a layout that has drifted from
        # include/lacx.h would otherwise show up as memory corruption behind the first call that fills one
        L.lacx_sizeof.restype = C.c_uint32
        L.lacx_sizeof.argtypes = [C.c_char_p]
        for name, cls in abi_structs().items():
            want = int(L.lacx_sizeof(name.encode()))
            if want != C.sizeof(cls):
                raise RuntimeError(f"{path}: sizeof(lacx_{name}) is {want}, the Python binding declares {C.sizeof(cls)} bytes")
        _libs[path] = L
        _lib = L
    return _lib


def abi_structs() -> dict:
    """include/lacx.h struct name (without the prefix) -> the ctypes class that mirrors it."""
    return {"config": Config, "channel_plan": ChannelPlan, "block_plan": BlockPlan, "timing": Timing, "pcm": Pcm,
            "batch_item": BatchItem, "batch_out": BatchOut, "wav_info": WavInfo, "fanout_shard": FanoutShard,
            "fanout_out": FanoutOut, "fanout_stats": FanoutStats, "stream_info": StreamInfo, "span": Span,
            "decode_item": DecodeItem, "window_item": WindowItem, "verify_item": VerifyItem,
            "verify_result": VerifyResult, "digest": Digest, "digest_source": DigestSource,
            "block_fault": BlockFault, "salvage_result": SalvageResult, "block_digest": BlockDigest,
            "manifest_info": ManifestInfo, "recovery_params": RecoveryParams, "recovery_info": RecoveryInfo,
            "repair_result": RepairResult, "channel_stats": ChannelStats, "block_stats": BlockStats,
            "channel_totals": ChannelTotals, "stats": Stats, "loudness_row": LoudnessRow, "loudness": Loudness,
            "truepeak_row": TruePeakRow, "truepeak_channel": TruePeakChannel, "truepeak": TruePeak,
            "ar_disc": ArDisc, "ar_id": ArId, "ar_result": ArResult, "ar_track": ArTrack, "compare_pair": ComparePair, "compare_channel_row": CompareChannelRow,
            "compare_row": CompareRow, "compare_channel": CompareChannel, "compare": Compare, "spectrum_row": SpectrumRow, "spectrum": Spectrum, "channel_info": ChannelInfo, "block_info": BlockInfo,
            "stream_report": StreamReport, "edit_segment": EditSegment, "edit_output": EditOutput,
            "edit_result": EditResult, "run_detector": RunDetector, "run_query": RunQuery, "run": Run,
            "run_totals": RunTotals, "runs_result": RunsResult}


def device_count() -> int:
    return int(lib().lacx_device_count())


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def _raise(handle, rc):
    msg = lib().lacx_last_error(handle).decode(errors="replace")
    if rc == E_INVALID:
        raise ValueError(msg)
    raise RuntimeError(msg)


def _take(ptr, size) -> bytes:
    data = C.string_at(ptr, size.value)
    lib().lacx_free(ptr)
    return data


class Encoder:
    """Mirror of LAC::Encoder (ref src/codec/lac/encoder.hpp:12-43)."""

    def __init__(self, order: int = 12, stereo_mode: int = 0, sample_rate: int = 44100, bit_depth: int = 16,
                 debug_lpc: bool = False, debug_stereo_est: bool = False, debug_zr: bool = False,
                 device: int = -1, devices=None, min_blocks_per_device: int = 0):
        """device: HIP ordinal, -1 = the current device, DEVICE_ALL = every visible device.  devices: an explicit device list
        (lacx_encoder_create_multi): encode / encode_wav / encode_wav_view spread the stream's blocks over them."""
        self.order = order  # stored and ignored, as in the reference (ref block/encoder.cpp:41)
        self._cfg = Config(sample_rate & 0xFFFFFFFF, bit_depth & 0xFF, stereo_mode & 0xFF, 1, 1, device, 0, 0)
        self._raw_stereo_mode = stereo_mode
        self._devices = None if devices is None else [int(d) for d in devices]
        self._min_blocks = int(min_blocks_per_device)
        self._h = None

    # -- setters of the reference ------------------------------------------------------------
    def set_zero_run_enabled(self, enabled: bool):
        self._cfg.zero_run_enabled = 1 if enabled else 0
        self._reset()

    def set_partitioning_enabled(self, enabled: bool):
        self._cfg.partitioning_enabled = 1 if enabled else 0
        self._reset()

    def set_debug_partitions(self, enabled: bool):  # debug prints only in the reference
        pass

    def set_thread_count(self, max_threads: int):
        self._cfg.emit_threads = int(max_threads)
        self._reset()

    def set_host_emit(self, enabled: bool):
        """True keeps the bit emit on the host (north_star layout); default is the device-side emit."""
        self._cfg.flags = (self._cfg.flags | 1) if enabled else (self._cfg.flags & ~1)
        self._reset()

    # -- plumbing ------------------------------------------------------------------------------
    def _reset(self):
        if self._h is not None:
            lib().lacx_encoder_destroy(self._h)
            self._h = None

    def _handle(self):
        if self._h is None:
            h = C.c_void_p()
            if self._devices is not None:
                devs = (C.c_int32 * len(self._devices))(*self._devices)
                rc = lib().lacx_encoder_create_multi(C.byref(self._cfg), devs, C.c_uint32(len(self._devices)),
                                                     C.c_uint32(self._min_blocks), C.byref(h))
            else:
                rc = lib().lacx_encoder_create(C.byref(self._cfg), C.byref(h))
            if rc != OK:
                raise RuntimeError("lacx_encoder_create failed")
            self._h = h
        return self._h

    # -- the fan-out over several devices ------------------------------------------------------------
    def lanes(self) -> int:
        return int(lib().lacx_encoder_lanes(self._handle()))

    def fanout_stats(self) -> "FanoutStats":
        st = FanoutStats()
        lib().lacx_get_fanout_stats(self._handle(), C.byref(st))
        return st

    def fanout_exchange_note(self) -> str:
        return lib().lacx_fanout_exchange_note(self._handle()).decode(errors="replace")

    def lane_timing(self, lane: int) -> Timing:
        t = Timing()
        if lib().lacx_get_lane_timing(self._handle(), C.c_uint32(lane), C.byref(t)) != OK:
            raise ValueError("no such lane")
        return t

    def encode_fanout_resident(self, shards):
        """shards: [(data_ptr, layout, channels, frames[, data1_ptr]), ...], shard g resident on the device of lane g.
        Returns [(PayloadView, table, device, byte_offset), ...] (views into the lanes' pinned result regions)."""
        n = len(shards)
        ins = (FanoutShard * n)()
        for it, sh in zip(ins, shards):
            it.pcm = Pcm(sh[0], sh[4] if len(sh) > 4 else None, sh[1], sh[2])
            it.frames = sh[3]
        outs = (FanoutOut * n)()
        h = self._handle()
        rc = lib().lacx_encode_fanout_resident(h, ins, C.c_uint32(n), outs)
        if rc != OK:
            _raise(h, rc)
        return [(PayloadView(o.payload, o.payload_size), np.ctypeslib.as_array(o.table, shape=(o.nblocks, 2)), int(o.device),
                 int(o.byte_offset)) for o in outs]

    def close(self):
        self._reset()

    def __del__(self):
        try:
            self._reset()
        except Exception:
            pass

    def timing(self) -> Timing:
        t = Timing()
        lib().lacx_get_timing(self._handle(), C.byref(t))
        return t

    # -- LAC::Encoder::encode ------------------------------------------------------------------
    def encode(self, left, right=None) -> bytes:
        L, lp = _i32(left)
        rp = None
        if right is not None and len(right) != 0:
            R, rp = _i32(right)
            if R.size != L.size:
                raise ValueError(f"right channel size ({R.size}) must match left channel size ({L.size})")
        if L.size == 0:
            raise ValueError("left channel must not be empty")
        out = C.POINTER(C.c_uint8)()
        size = C.c_uint64()
        h = self._handle()
        rc = lib().lacx_encode(h, lp, rp, C.c_uint64(L.size), C.byref(out), C.byref(size))
        if rc != OK:
            _raise(h, rc)
        return _take(out, size)

    def analyze(self, left, right=None):
        """Device analysis only: (block_plans, channel_plans[nblocks*16]) as ctypes arrays."""
        L, lp = _i32(left)
        rp = None
        if right is not None:
            R, rp = _i32(right)
        nb = (L.size + MAX_BLOCK - 1) // MAX_BLOCK
        bplans = (BlockPlan * nb)()
        plans = (ChannelPlan * (nb * SLOTS))()
        h = self._handle()
        rc = lib().lacx_analyze(h, lp, rp, C.c_uint64(L.size), bplans, plans)
        if rc != OK:
            _raise(h, rc)
        return bplans, plans

    def emit_from_plans(self, left, right, bplans, plans) -> bytes:
        """Host-only emit + container from plan records (no device involved)."""
        L, lp = _i32(left)
        rp = None
        if right is not None:
            R, rp = _i32(right)
        out = C.POINTER(C.c_uint8)()
        size = C.c_uint64()
        h = self._handle()
        rc = lib().lacx_emit_from_plans(h, lp, rp, C.c_uint64(L.size), bplans, plans, C.byref(out), C.byref(size))
        if rc != OK:
            _raise(h, rc)
        return _take(out, size)

    def encode_shard(self, left, right=None):
        """Block-range shard: (payload bytes, table uint32[nblocks,2])."""
        L, lp = _i32(left)
        rp = None
        if right is not None:
            R, rp = _i32(right)
        pay = C.POINTER(C.c_uint8)()
        psize = C.c_uint64()
        tab = C.POINTER(C.c_uint32)()
        nb = C.c_uint32()
        h = self._handle()
        rc = lib().lacx_encode_shard(h, lp, rp, C.c_uint64(L.size), C.byref(pay), C.byref(psize), C.byref(tab),
                                     C.byref(nb))
        if rc != OK:
            _raise(h, rc)
        table = np.ctypeslib.as_array(tab, shape=(nb.value, 2)).copy()
        lib().lacx_free(tab)
        return _take(pay, psize), table

    # device-resident entry points (raw pointers; torch tensors welcome) -----------------------
    def encode_device(self, d_left_ptr: int, d_right_ptr: int | None, h_left, h_right, frames: int,
                      stream: int = 0) -> bytes:
        hl, hlp = _i32(h_left)
        hrp = None
        if h_right is not None:
            hr, hrp = _i32(h_right)
        out = C.POINTER(C.c_uint8)()
        size = C.c_uint64()
        h = self._handle()
        rc = lib().lacx_encode_device(h, C.c_void_p(d_left_ptr), C.c_void_p(d_right_ptr or 0), hlp, hrp,
                                      C.c_uint64(frames), C.c_void_p(stream), C.byref(out), C.byref(size))
        if rc != OK:
            _raise(h, rc)
        return _take(out, size)

    def analyze_device(self, d_left_ptr: int, d_right_ptr: int | None, frames: int, stream: int = 0, plans: bool = False):
        """Runs the kernels on device-resident PCM.  plans=False: returns nothing (the records stay in the encoder);
        plans=True: (block_plans, channel_plans[nblocks*16]) as lacx_analyze returns them."""
        h = self._handle()
        bplans = cplans = None
        if plans:
            nb = (frames + MAX_BLOCK - 1) // MAX_BLOCK
            bplans = (BlockPlan * nb)()
            cplans = (ChannelPlan * (nb * SLOTS))()
        rc = lib().lacx_analyze_device(h, C.c_void_p(d_left_ptr), C.c_void_p(d_right_ptr or 0), C.c_uint64(frames),
                                       C.c_void_p(stream), bplans, cplans)
        if rc != OK:
            _raise(h, rc)
        if plans:
            return bplans, cplans

    def encode_shard_device_view(self, d_left_ptr: int, d_right_ptr: int | None, h_left, h_right, frames: int,
                                 stream: int = 0):
        """Zero-copy shard encode: (PayloadView, table) backed by encoder-owned pinned memory."""
        hl, hlp = _i32(h_left)
        hrp = None
        if h_right is not None:
            hr, hrp = _i32(h_right)
        pay = C.POINTER(C.c_uint8)()
        psize = C.c_uint64()
        tab = C.POINTER(C.c_uint32)()
        nb = C.c_uint32()
        h = self._handle()
        rc = lib().lacx_encode_shard_device_view(h, C.c_void_p(d_left_ptr), C.c_void_p(d_right_ptr or 0), hlp, hrp,
                                                 C.c_uint64(frames), C.c_void_p(stream), C.byref(pay),
                                                 C.byref(psize), C.byref(tab), C.byref(nb))
        if rc != OK:
            _raise(h, rc)
        table = np.ctypeslib.as_array(tab, shape=(nb.value, 2))
        return PayloadView(pay, psize.value), table

    def encode_shard_pcm_device_begin(self, data_ptr, layout: int | None = None, channels: int | None = None,
                                      frames: int | None = None, stream: int = 0, data1_ptr: int | None = None):
        """Enqueues a shard encode of device-resident PCM and returns at once (see encode_shard_end).  data_ptr: a raw
        device address with its layout, channel count and frame count, or a device tensor (see pcm_of) by itself."""
        pcm, frames = _pcm_arg(data_ptr, layout, channels, frames, data1_ptr, self._cfg.bit_depth)
        h = self._handle()
        rc = lib().lacx_encode_shard_pcm_device_begin(h, C.byref(pcm), C.c_uint64(frames), C.c_void_p(stream))
        if rc != OK:
            _raise(h, rc)

    def encode_shard_end(self):
        """Waits for the encode started by encode_shard_pcm_device_begin: (PayloadView, table)."""
        pay = C.POINTER(C.c_uint8)()
        psize = C.c_uint64()
        tab = C.POINTER(C.c_uint32)()
        nb = C.c_uint32()
        h = self._handle()
        rc = lib().lacx_encode_shard_end(h, C.byref(pay), C.byref(psize), C.byref(tab), C.byref(nb))
        if rc != OK:
            _raise(h, rc)
        table = np.ctypeslib.as_array(tab, shape=(nb.value, 2))
        return PayloadView(pay, psize.value), table

    def encode_wav(self, wav: bytes) -> bytes:
        """Complete .lac of a PCM WAV file image: the raw data chunk goes to the device as it is (ref
        src/io/wav_io.cpp:167-277 + src/main.cpp:640-675 chained)."""
        out = C.POINTER(C.c_uint8)()
        size = C.c_uint64()
        h = self._handle()
        view = np.frombuffer(wav, dtype=np.uint8)  # no copy: the library only reads the image
        rc = lib().lacx_encode_wav(h, view.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint64(view.size), C.byref(out),
                                   C.byref(size))
        if rc != OK:
            _raise(h, rc)
        try:
            return C.string_at(out, size.value)
        finally:
            lib().lacx_free(out)

    def encode_wav_view(self, wav) -> "PayloadView":
        """Zero-copy form of encode_wav: a view of the complete .lac in the encoder's pinned result buffer (valid until
        the encoder's next call); `wav` is any buffer (bytes, numpy uint8 array, mmap)."""
        out = C.POINTER(C.c_uint8)()
        size = C.c_uint64()
        h = self._handle()
        view = np.frombuffer(wav, dtype=np.uint8)
        rc = lib().lacx_encode_wav_view(h, view.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint64(view.size), C.byref(out),
                                        C.byref(size))
        if rc != OK:
            _raise(h, rc)
        return PayloadView(out, size.value)

    def encode_shard_pcm_device_view(self, data_ptr, layout: int | None = None, channels: int | None = None,
                                     frames: int | None = None, stream: int = 0, data1_ptr: int | None = None):
        """Zero-copy shard encode of device-resident PCM in its source layout (any PCM_* layout).  data_ptr: a raw device
        address with its layout, channel count and frame count, or a device tensor (see pcm_of) by itself."""
        pcm, frames = _pcm_arg(data_ptr, layout, channels, frames, data1_ptr, self._cfg.bit_depth)
        pay = C.POINTER(C.c_uint8)()
        psize = C.c_uint64()
        tab = C.POINTER(C.c_uint32)()
        nb = C.c_uint32()
        h = self._handle()
        rc = lib().lacx_encode_shard_pcm_device_view(h, C.byref(pcm), C.c_uint64(frames), C.c_void_p(stream),
                                                     C.byref(pay), C.byref(psize), C.byref(tab), C.byref(nb))
        if rc != OK:
            _raise(h, rc)
        table = np.ctypeslib.as_array(tab, shape=(nb.value, 2))
        return PayloadView(pay, psize.value), table

    def encode_tensor(self, t, stream: int = 0) -> bytes:
        """The complete .lac of a device tensor ([channels, frames], [frames, channels] or [frames]; int16, int32 or
        float32, see pcm_of) at the encoder's rate, depth and stereo mode: a shard encode of the tensor where it lies,
        then the container around it.  A float that is no exact sample of the depth raises ValueError."""
        pcm, _ = pcm_of(t, self._cfg.bit_depth)
        payload, table = self.encode_shard_pcm_device_view(t, stream=stream)
        return assemble(self._cfg.sample_rate, self._cfg.bit_depth, self._cfg.stereo_mode, int(pcm.channels),
                        [(payload.tobytes(), table)])

    def encode_shard_device(self, d_left_ptr: int, d_right_ptr: int | None, h_left, h_right, frames: int,
                            stream: int = 0, copy: bool = True):
        """Shard encode of device-resident PCM. With copy=False the payload comes back as a zero-copy
        `Payload` view of the library's buffer (freed when the object dies)."""
        hl, hlp = _i32(h_left)
        hrp = None
        if h_right is not None:
            hr, hrp = _i32(h_right)
        pay = C.POINTER(C.c_uint8)()
        psize = C.c_uint64()
        tab = C.POINTER(C.c_uint32)()
        nb = C.c_uint32()
        h = self._handle()
        rc = lib().lacx_encode_shard_device(h, C.c_void_p(d_left_ptr), C.c_void_p(d_right_ptr or 0), hlp, hrp,
                                            C.c_uint64(frames), C.c_void_p(stream), C.byref(pay), C.byref(psize),
                                            C.byref(tab), C.byref(nb))
        if rc != OK:
            _raise(h, rc)
        table = np.ctypeslib.as_array(tab, shape=(nb.value, 2)).copy()
        lib().lacx_free(tab)
        if not copy:
            return Payload(pay, psize.value), table
        return _take(pay, psize), table


class Pcm(C.Structure):
    _fields_ = [("data0", C.c_void_p), ("data1", C.c_void_p), ("layout", C.c_uint32), ("channels", C.c_uint32)]


class FanoutShard(C.Structure):
    _fields_ = [("pcm", Pcm), ("frames", C.c_uint64)]


class FanoutOut(C.Structure):
    _fields_ = [("payload", C.POINTER(C.c_uint8)), ("payload_size", C.c_uint64), ("table", C.POINTER(C.c_uint32)),
                ("nblocks", C.c_uint32), ("device", C.c_int32), ("byte_offset", C.c_uint64)]


EXCHANGE_HOST, EXCHANGE_RCCL = 1, 2


class FanoutStats(C.Structure):
    _fields_ = [("lanes_used", C.c_uint32), ("exchange", C.c_uint32), ("exchange_ms", C.c_double), ("concat_ms", C.c_double),
                ("device", C.c_int32 * MAX_FANOUT), ("blocks", C.c_uint32 * MAX_FANOUT), ("lane_frames", C.c_uint64 * MAX_FANOUT),
                ("payload_bytes", C.c_uint64 * MAX_FANOUT), ("encode_ms", C.c_double * MAX_FANOUT)]


def fanout_range(nblocks: int, nlanes: int, lane: int):
    """(first block, block count) of lane `lane` of `nlanes` over a stream of `nblocks` blocks."""
    a, b = C.c_uint32(), C.c_uint32()
    lib().lacx_fanout_range(C.c_uint32(nblocks), C.c_uint32(nlanes), C.c_uint32(lane), C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


PCM_PLANAR_I32, PCM_INTERLEAVED_I16, PCM_INTERLEAVED_I24 = 0, 1, 2
PCM_PLANAR_I16, PCM_PLANAR_F32, PCM_INTERLEAVED_F32 = 16, 17, 18  # the tensor layouts


def pcm_of(x, bit_depth: int):
    """(Pcm, frames) of an array where it lies: a numpy array (the host-side twins) or anything with data_ptr(), dtype,
    shape and stride() -- a torch tensor, which this module does not import.
      [channels, frames] with contiguous rows   planar: data1 is the second row's address (a slice of a wider tensor is fine)
      [frames, channels] contiguous             interleaved;  [frames]: mono
      int32 -> PCM_PLANAR_I32, int16 -> PCM_PLANAR_I16 (interleaved: PCM_INTERLEAVED_I16), float32 -> PCM_PLANAR_F32 /
      PCM_INTERLEAVED_F32 (sample * 2^-(bit_depth - 1), what decode_window_batch_device writes)
    A two-dimensional array whose first extent is 1 or 2 is taken as [channels, frames].  Everything else raises
    ValueError with the reason: another dtype, more than two channels, a non-unit inner stride, rows that overlap,
    interleaved int32, int16 at a depth other than 16, an empty array."""
    if isinstance(x, np.ndarray):
        ptr, dtype, shape = int(x.ctypes.data), x.dtype.name, tuple(x.shape)
        strides = tuple(s // x.itemsize if s % x.itemsize == 0 else None for s in x.strides)
    elif all(hasattr(x, a) for a in ("data_ptr", "dtype", "shape", "stride")):
        ptr, dtype, shape = int(x.data_ptr()), str(x.dtype).replace("torch.", ""), tuple(int(n) for n in x.shape)
        strides = tuple(int(n) for n in x.stride())
    else:
        raise ValueError(f"pcm_of: {type(x).__name__} is neither a numpy array nor a tensor with data_ptr(), dtype, shape and stride()")
    size = {"int16": 2, "int32": 4, "float32": 4}.get(dtype)
    if size is None:
        raise ValueError(f"pcm_of: dtype {dtype} is not int16, int32 or float32")
    if dtype == "int16" and bit_depth != 16:
        raise ValueError(f"pcm_of: int16 samples need bit depth 16, not {bit_depth}")
    if len(shape) not in (1, 2) or 0 in shape:
        raise ValueError(f"pcm_of: shape {shape} is not [channels, frames], [frames, channels] or [frames], or is empty")
    if None in strides or any(s < 0 for s in strides):
        raise ValueError(f"pcm_of: strides {strides} are not whole, non-negative element counts")
    planar = {"int16": PCM_PLANAR_I16, "int32": PCM_PLANAR_I32, "float32": PCM_PLANAR_F32}[dtype]
    if len(shape) == 1:
        if shape[0] > 1 and strides[0] != 1:
            raise ValueError(f"pcm_of: inner stride {strides[0]} is not 1")
        return Pcm(ptr, None, planar, 1), shape[0]
    if shape[0] <= 2:  # [channels, frames]
        ch, frames = shape
        if frames > 1 and strides[1] != 1:
            raise ValueError(f"pcm_of: inner stride {strides[1]} is not 1")
        if ch == 2 and strides[0] < frames:
            raise ValueError(f"pcm_of: row stride {strides[0]} is shorter than a row of {frames} frames")
        return Pcm(ptr, ptr + strides[0] * size if ch == 2 else None, planar, ch), frames
    frames, ch = shape  # [frames, channels]
    if ch > 2:
        raise ValueError(f"pcm_of: more than two channels (shape {shape})")
    if strides != (ch, 1):
        raise ValueError(f"pcm_of: [frames, channels] must be contiguous, strides are {strides}")
    if ch == 1:
        return Pcm(ptr, None, planar, 1), frames
    if dtype == "int32":
        raise ValueError("pcm_of: interleaved int32 is not a supported layout")
    return Pcm(ptr, None, PCM_INTERLEAVED_I16 if dtype == "int16" else PCM_INTERLEAVED_F32, 2), frames


def _pcm_arg(data, layout, channels, frames, data1_ptr, bit_depth):
    """(Pcm, frames) of an entry point's PCM argument: a raw address with its description, or a tensor by itself."""
    if isinstance(data, (int, np.integer)) or data is None:
        if layout is None or channels is None or frames is None:
            raise ValueError("a raw device address needs its layout, channel count and frame count")
        return Pcm(data, data1_ptr, layout, channels), int(frames)
    if not (layout is None and channels is None and frames is None and data1_ptr is None):
        raise ValueError("a tensor describes itself: layout, channels, frames and data1_ptr must not be given")
    return pcm_of(data, bit_depth)


class PayloadView:
    """Borrowed view of encoder-owned pinned memory (valid until the encoder's next call)."""

    def __init__(self, ptr, size):
        self._ptr = ptr
        self.size = size

    def __len__(self):
        return self.size

    def tobytes(self) -> bytes:
        return C.string_at(self._ptr, self.size)


class Payload:
    """Zero-copy view of a malloc'd library buffer."""

    def __init__(self, ptr, size):
        self._ptr = ptr
        self.size = size

    def __len__(self):
        return self.size

    def array(self) -> np.ndarray:
        return np.ctypeslib.as_array(self._ptr, shape=(self.size,)) if self.size else np.zeros(0, np.uint8)

    def tobytes(self) -> bytes:
        return C.string_at(self._ptr, self.size)

    def __del__(self):
        try:
            if self._ptr is not None:
                lib().lacx_free(self._ptr)
                self._ptr = None
        except Exception:
            pass


class WavInfo(C.Structure):
    _fields_ = [("channels", C.c_uint16), ("bit_depth", C.c_uint16), ("sample_rate", C.c_uint32),
                ("frames", C.c_uint64), ("data_offset", C.c_uint64), ("data_bytes", C.c_uint64)]


def wav_parse(wav: bytes):
    """RIFF walk with the reference's accept/reject rules (ref src/io/wav_io.cpp:167-277); None when rejected.
    Host-only: needs no device."""
    info = WavInfo()
    buf = (C.c_uint8 * max(1, len(wav))).from_buffer_copy(wav if wav else b"\0")
    rc = lib().lacx_wav_parse(buf, C.c_uint64(len(wav)), C.byref(info))
    return info if rc == OK else None


class StreamInfo(C.Structure):
    _fields_ = [("sample_rate", C.c_uint32), ("blocks", C.c_uint32), ("frames", C.c_uint64), ("channels", C.c_uint8),
                ("bit_depth", C.c_uint8), ("stereo_mode", C.c_uint8), ("version", C.c_uint8)]


class Span(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_uint8)), ("size", C.c_uint64)]


class DecodeItem(C.Structure):
    _fields_ = [("lac", C.POINTER(C.c_uint8)), ("size", C.c_uint64), ("left", C.c_void_p), ("right", C.c_void_p),
                ("frames", C.c_uint64)]


class WindowItem(C.Structure):
    _fields_ = [("lac", C.POINTER(C.c_uint8)), ("size", C.c_uint64), ("start", C.c_uint64), ("frames", C.c_uint64),
                ("left", C.c_void_p), ("right", C.c_void_p)]


class VerifyItem(C.Structure):
    _fields_ = [("lac", C.POINTER(C.c_uint8)), ("size", C.c_uint64), ("pcm", Pcm), ("frames", C.c_uint64)]


class VerifyResult(C.Structure):
    """mismatches == 0: the stream decodes to exactly its source; else the first differing sample (lowest frame, then
    lowest channel), its block in the stream and the two values there."""
    _fields_ = [("mismatches", C.c_uint64), ("frame", C.c_uint64), ("block", C.c_uint32), ("channel", C.c_uint8),
                ("reserved", C.c_uint8 * 3), ("decoded", C.c_int32), ("source", C.c_int32)]


class Digest(C.Structure):
    """CRC-32 (zlib.crc32) of what a stream decodes to, or of source PCM: data_crc32 over the bytes of the WAV data chunk
    (interleaved little-endian, bit_depth / 8 per sample), wav_crc32 over the whole canonical WAV file image (0 with
    wav_valid == 0: an image beyond the RIFF limit), and the format those bytes have."""
    _fields_ = [("data_crc32", C.c_uint32), ("wav_crc32", C.c_uint32), ("frames", C.c_uint64), ("data_bytes", C.c_uint64),
                ("sample_rate", C.c_uint32), ("channels", C.c_uint8), ("bit_depth", C.c_uint8), ("wav_valid", C.c_uint8),
                ("reserved", C.c_uint8)]


class DigestSource(C.Structure):
    _fields_ = [("pcm", Pcm), ("frames", C.c_uint64), ("sample_rate", C.c_uint32), ("bit_depth", C.c_uint8),
                ("reserved", C.c_uint8 * 3)]


BLOCK_MISSING = 10                           # LACX_BLOCK_MISSING
SALVAGE_TRUNCATED, SALVAGE_TRAILING = 1, 2   # LACX_SALVAGE_*


class BlockFault(C.Structure):
    """A lost block of a salvage decode: its number and first frame in the stream, its frames, and why (1..10)."""
    _fields_ = [("block", C.c_uint32), ("code", C.c_uint32), ("frame", C.c_uint64), ("frames", C.c_uint32),
                ("reserved", C.c_uint32)]

    @property
    def text(self) -> str:
        return block_fault_text(self.code)


class SalvageResult(C.Structure):
    """How much of a stream a salvage decode lost: first_bad == blocks when nothing; flags: SALVAGE_*."""
    _fields_ = [("blocks", C.c_uint32), ("bad_blocks", C.c_uint32), ("frames", C.c_uint64), ("lost_frames", C.c_uint64),
                ("first_bad", C.c_uint32), ("flags", C.c_uint32)]


BLOCK_DIGEST = 11                            # LACX_BLOCK_DIGEST: the block decodes, but not to what its manifest says


class BlockDigest(C.Structure):
    """One block of a stream or of source PCM: its frames and the CRC-32 (zlib.crc32) of the bytes it has in the WAV data
    chunk; code != 0: the block is lost (1..10) and crc32 is 0."""
    _fields_ = [("frames", C.c_uint32), ("crc32", C.c_uint32), ("code", C.c_uint32), ("reserved", C.c_uint32)]


class ManifestInfo(C.Structure):
    _fields_ = [("sample_rate", C.c_uint32), ("blocks", C.c_uint32), ("frames", C.c_uint64), ("data_crc32", C.c_uint32),
                ("channels", C.c_uint8), ("bit_depth", C.c_uint8), ("reserved", C.c_uint8 * 2)]


# ---- audio statistics: exact integers from the device; the float conveniences are DERIVED here and documented as such ----
def _wasted_bits(or_bits: int, depth: int) -> int:
    """Trailing zero bits of an OR of samples; the whole depth where it is 0 (silence uses no bit)."""
    return depth if or_bits == 0 else (or_bits & -or_bits).bit_length() - 1


def _dbfs(ratio: float) -> float:
    return 20.0 * math.log10(ratio) if ratio > 0 else float("-inf")


class ChannelStats(C.Structure):
    """One channel of one block: min, max, OR of the samples' low bits, the counts of full-scale and of zero samples, the
    sum and the sum of squares -- all exact."""
    _fields_ = [("min", C.c_int32), ("max", C.c_int32), ("or_bits", C.c_uint32), ("full_scale", C.c_uint32), ("zeros", C.c_uint32),
                ("reserved", C.c_uint32), ("sum", C.c_int64), ("sum_sq", C.c_uint64)]

    @property
    def peak(self) -> int:
        return max(abs(self.min), abs(self.max))


class BlockStats(C.Structure):
    """One block of a stream or of source PCM.  code != 0: the block is lost (1..10) and every other field but frames is
    0.  lead_zero_frames / trail_zero_frames: leading / trailing frames that are 0 in every channel (both == frames for a
    silent block); differing: frames with left != right."""
    _fields_ = [("frames", C.c_uint32), ("code", C.c_uint32), ("lead_zero_frames", C.c_uint32), ("trail_zero_frames", C.c_uint32),
                ("differing", C.c_uint32), ("reserved", C.c_uint32), ("ch", ChannelStats * 2)]

    @property
    def silent(self) -> bool:
        return self.code == 0 and self.lead_zero_frames == self.frames


class ChannelTotals(C.Structure):
    """One channel of an item: as ChannelStats, the sums 128 bits wide (`sum` and `sum_sq` give them as Python ints)."""
    _fields_ = [("min", C.c_int32), ("max", C.c_int32), ("or_bits", C.c_uint32), ("reserved", C.c_uint32), ("full_scale", C.c_uint64),
                ("zeros", C.c_uint64), ("sum_lo", C.c_uint64), ("sum_hi", C.c_int64), ("sum_sq_lo", C.c_uint64), ("sum_sq_hi", C.c_uint64)]

    @property
    def sum(self) -> int:
        return (self.sum_hi << 64) + self.sum_lo

    @property
    def sum_sq(self) -> int:
        return (self.sum_sq_hi << 64) + self.sum_sq_lo

    @property
    def peak(self) -> int:
        return max(abs(self.min), abs(self.max))


class Stats(C.Structure):
    """The totals of an item over its decoded blocks (lacx_stats).  Exact: every field, `peak`, `wasted_bits`, `dual_mono`
    and the channels' `sum` / `sum_sq`.  Derived floats, not part of any equality: `peak_dbfs`, `rms_dbfs`, `dc`."""
    _fields_ = [("frames", C.c_uint64), ("sample_rate", C.c_uint32), ("channels", C.c_uint8), ("bit_depth", C.c_uint8),
                ("reserved", C.c_uint8 * 2), ("blocks", C.c_uint32), ("lost_blocks", C.c_uint32), ("lost_frames", C.c_uint64),
                ("silent_blocks", C.c_uint32), ("reserved2", C.c_uint32), ("lead_zero_frames", C.c_uint64),
                ("trail_zero_frames", C.c_uint64), ("differing", C.c_uint64), ("ch", ChannelTotals * 2)]

    @property
    def peak(self) -> int:
        return max(self.ch[c].peak for c in range(self.channels)) if self.channels else 0

    @property
    def wasted_bits(self) -> int:
        bits = 0
        for c in range(self.channels):
            bits |= self.ch[c].or_bits
        return _wasted_bits(bits, self.bit_depth)

    @property
    def dual_mono(self) -> bool:
        return self.channels == 2 and self.differing == 0

    @property
    def decoded_frames(self) -> int:
        return self.frames - self.lost_frames

    @property
    def peak_dbfs(self) -> float:
        """Derived: 20 log10(peak / 2^(b-1)); -inf for silence."""
        return _dbfs(self.peak / float(1 << (self.bit_depth - 1))) if self.bit_depth else float("-inf")

    def rms_dbfs(self, channel: int = 0) -> float:
        """Derived: the channel's RMS over the decoded frames against full scale, in dB; -inf for silence."""
        n = self.decoded_frames
        if n == 0 or not self.bit_depth:
            return float("-inf")
        return _dbfs(math.sqrt(self.ch[channel].sum_sq / n) / float(1 << (self.bit_depth - 1)))

    def dc(self, channel: int = 0) -> float:
        """Derived: the channel's mean over the decoded frames / 2^(b-1)."""
        n = self.decoded_frames
        return self.ch[channel].sum / n / float(1 << (self.bit_depth - 1)) if n and self.bit_depth else 0.0


# ---- loudness: BS.1770 integrated, momentary, short-term and range (lacx.h) ----
LOUDNESS_TOO_SHORT, LOUDNESS_SILENT = 1, 2  # LACX_LOUDNESS_*


class LoudnessRow(C.Structure):
    """One sub-block of sample_rate / 10 frames: the K-weighted energy per channel (lacx_loudness_row)."""
    _fields_ = [("energy", C.c_double * 2)]


class Loudness(C.Structure):
    """The loudness of an item or an album (lacx_loudness): levels in LUFS, `range_lu` in LU; -inf where lacx.h says so.
    `gain` = -18 - integrated, the ReplayGain 2 reference, as a number only: nothing is ever applied to the audio."""
    _fields_ = [("frames", C.c_uint64), ("sample_rate", C.c_uint32), ("channels", C.c_uint8), ("bit_depth", C.c_uint8), ("flags", C.c_uint8),
                ("reserved", C.c_uint8), ("subblocks", C.c_uint32), ("gating_blocks", C.c_uint32), ("above_absolute", C.c_uint32),
                ("above_relative", C.c_uint32), ("integrated_lufs", C.c_double), ("relative_gate_lufs", C.c_double),
                ("momentary_max_lufs", C.c_double), ("shortterm_max_lufs", C.c_double), ("range_lu", C.c_double)]

    @property
    def too_short(self) -> bool:
        return bool(self.flags & LOUDNESS_TOO_SHORT)

    @property
    def silent(self) -> bool:
        return bool(self.flags & LOUDNESS_SILENT)

    @property
    def gain(self) -> float:
        return -18.0 - self.integrated_lufs


def loudness_combine(sets) -> Loudness:
    """Host only: the loudness of [(rows, channels, bit_depth, sample_rate)] -- one set gives an item's totals as
    loudness_batch makes them, several give album loudness (lacx.h).  rows: LoudnessRow records or an (S, 2) array."""
    n = len(sets)
    arrays = []
    for rows, _, _, _ in sets:
        if isinstance(rows, np.ndarray):
            a = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, 2))
        elif isinstance(rows, C.Array):  # what loudness_batch hands out
            a = np.frombuffer(bytes(rows), dtype=np.float64).reshape(-1, 2)
        else:
            a = np.array([[r.energy[0], r.energy[1]] for r in rows], dtype=np.float64).reshape(-1, 2)
        arrays.append(a)
    ptrs = (C.POINTER(LoudnessRow) * max(1, n))(*[C.cast(a.ctypes.data, C.POINTER(LoudnessRow)) for a in arrays])
    counts = (C.c_uint32 * max(1, n))(*[len(a) for a in arrays])
    channels = (C.c_uint8 * max(1, n))(*[s[1] for s in sets])
    depths = (C.c_uint8 * max(1, n))(*[s[2] for s in sets])
    rates = (C.c_uint32 * max(1, n))(*[s[3] for s in sets])
    out = Loudness()
    if lib().lacx_loudness_combine(ptrs, counts, channels, depths, rates, C.c_uint32(n), C.byref(out)) != OK:
        raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
    return out


# ---- true peak: the BS.1770 maximum of the 4x oversampled signal (lacx.h) ----
TRUEPEAK_OVER, TRUEPEAK_SAMPLE_FULL = 1, 2  # LACX_TRUEPEAK_*
TRUEPEAK_ROW_FRAMES = 16384


class TruePeakRow(C.Structure):
    """One segment of 16384 frames: per channel max |y| of the oversampled signal times 8192, its first position inside the
    row as 4 * frame + phase, and the largest sample (lacx_truepeak_row)."""
    _fields_ = [("peak", C.c_uint64 * 2), ("pos", C.c_uint32 * 2), ("sample_peak", C.c_uint32 * 2)]


class TruePeakChannel(C.Structure):
    _fields_ = [("peak", C.c_uint64), ("position", C.c_uint64), ("sample_peak", C.c_uint32), ("sample_peak_row", C.c_uint32)]


class TruePeak(C.Structure):
    """The true peak of an item or an album (lacx_truepeak): `true_peak` linear (what a REPLAYGAIN_*_PEAK tag holds),
    `true_peak_dbtp` and `sample_peak_dbfs` in dB, -inf for all-zero audio.  Nothing is ever applied to the audio."""
    _fields_ = [("frames", C.c_uint64), ("sample_rate", C.c_uint32), ("channels", C.c_uint8), ("bit_depth", C.c_uint8), ("flags", C.c_uint8),
                ("peak_channel", C.c_uint8), ("rows", C.c_uint32), ("set", C.c_uint32), ("ch", TruePeakChannel * 2),
                ("true_peak", C.c_double), ("true_peak_dbtp", C.c_double), ("sample_peak_dbfs", C.c_double)]

    @property
    def over(self) -> bool:
        return bool(self.flags & TRUEPEAK_OVER)

    @property
    def sample_full(self) -> bool:
        return bool(self.flags & TRUEPEAK_SAMPLE_FULL)

    @property
    def position(self) -> int:
        """4 * frame + phase of the peak in the stream (of the winning set for an album)."""
        return int(self.ch[self.peak_channel].position)


def truepeak_combine(sets) -> TruePeak:
    """Host only: the true peak of [(rows, channels, bit_depth, frames, sample_rate)] -- one set gives an item's totals as
    truepeak_batch makes them, several give the album peak (lacx.h).  rows: TruePeakRow records or their bytes."""
    n = len(sets)
    blobs = []
    for rows, _, _, _, _ in sets:
        raw = bytes(rows) if isinstance(rows, (C.Array, bytes, bytearray, np.ndarray)) else b"".join(bytes(r) for r in rows)
        blobs.append(np.frombuffer(raw, dtype=np.uint8).copy())
    ptrs = (C.POINTER(TruePeakRow) * max(1, n))(*[C.cast(a.ctypes.data, C.POINTER(TruePeakRow)) for a in blobs])
    counts = (C.c_uint32 * max(1, n))(*[len(a) // C.sizeof(TruePeakRow) for a in blobs])
    channels = (C.c_uint8 * max(1, n))(*[s[1] for s in sets])
    depths = (C.c_uint8 * max(1, n))(*[s[2] for s in sets])
    frames = (C.c_uint64 * max(1, n))(*[s[3] for s in sets])
    rates = (C.c_uint32 * max(1, n))(*[s[4] for s in sets])
    out = TruePeak()
    if lib().lacx_truepeak_combine(ptrs, counts, channels, depths, frames, rates, C.c_uint32(n), C.byref(out)) != OK:
        raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
    return out


# ---- spectrum: the long-term power spectrum in 64 bands and the bandwidth (lacx.h) ----
SPECTRUM_WINDOWS = (256, 512, 1024, 2048, 4096)
SPECTRUM_BANDS = 64
SPECTRUM_ROW_FRAMES = 16384


class SpectrumRow(C.Structure):
    """One segment of 16384 frames: per channel and band the summed one-sided power of the Hann windows whose first frame
    lies in it (lacx_spectrum_row)."""
    _fields_ = [("power", (C.c_double * 64) * 2)]


class Spectrum(C.Structure):
    """The long-term spectrum of an item (lacx_spectrum): per channel `level_db[64]` in dB relative to a full-scale sine (-inf
    for a zero band), `bandwidth_hz` (the upper edge of the highest band at or above `floor_db`, 0 when none is) and
    `peak_band`.  It only measures."""
    _fields_ = [("frames", C.c_uint64), ("windows", C.c_uint64), ("sample_rate", C.c_uint32), ("window", C.c_uint32), ("rows", C.c_uint32),
                ("channels", C.c_uint8), ("bit_depth", C.c_uint8), ("peak_band", C.c_uint8 * 2), ("floor_db", C.c_double),
                ("bandwidth_hz", C.c_double * 2), ("level_db", (C.c_double * 64) * 2)]

    def peak_hz(self, channel: int) -> float:
        """The centre of the channel's strongest band."""
        return (self.peak_band[channel] + 0.5) * self.sample_rate / (2.0 * SPECTRUM_BANDS)


def spectrum_combine(rows, channels, bit_depth, frames, sample_rate, window=2048, floor_db=-100.0) -> Spectrum:
    """Host only: the totals of one item's rows as spectrum_batch makes them (lacx.h).  rows: SpectrumRow records or their
    bytes."""
    raw = bytes(rows) if isinstance(rows, (C.Array, bytes, bytearray, np.ndarray)) else b"".join(bytes(r) for r in rows)
    blob = np.frombuffer(raw, dtype=np.uint8).copy()
    out = Spectrum()
    if lib().lacx_spectrum_combine(C.cast(blob.ctypes.data, C.POINTER(SpectrumRow)), C.c_uint32(len(blob) // C.sizeof(SpectrumRow)), C.c_uint8(channels),
                                   C.c_uint8(bit_depth), C.c_uint64(frames), C.c_uint32(sample_rate), C.c_uint32(window), C.c_double(floor_db),
                                   C.byref(out)) != OK:
        raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
    return out


# ---- rip checksums: AccurateRip v1 / v2 at every read offset (lacx.h) ----
AR_FIRST, AR_LAST, AR_NO_IDS = 1, 2, 4  # LACX_AR_*
AR_TRACK_SHORT, AR_TRACK_NO_S450 = 1, 2
AR_MAX_RADIUS = 2939


class ArDisc(C.Structure):
    _fields_ = [("first_source", C.c_uint32), ("sources", C.c_uint32), ("first_track", C.c_uint32), ("tracks", C.c_uint32),
                ("flags", C.c_uint32), ("radius", C.c_uint32), ("lba0", C.c_uint32)]


class ArId(C.Structure):
    """The ids a rip database files a disc under (lacx_ar_id); all zero where the disc has none."""
    _fields_ = [("id1", C.c_uint32), ("id2", C.c_uint32), ("cddb", C.c_uint32)]


class ArResult(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("tracks", C.c_uint32), ("radius", C.c_uint32), ("flags", C.c_uint32), ("ids", ArId)]


class ArTrack(C.Structure):
    """One track: its first disc frame, frames, LACX_AR_TRACK_* flags and the three sums at offset 0 (lacx_ar_track)."""
    _fields_ = [("start", C.c_uint64), ("frames", C.c_uint64), ("flags", C.c_uint32), ("v1", C.c_uint32), ("v2", C.c_uint32), ("s450", C.c_uint32)]


class AccurateRip:
    """The rip checksums of one disc: `v1`, `v2`, `s450` as (tracks, 2 radius + 1) uint32 arrays ordered by `offsets` (-radius
    .. radius), `tracks` ([ArTrack]), `ids` (ArId), `frames`, `radius`, `flags`."""

    def __init__(self, result, tracks, v1, v2, s450):
        self.frames, self.radius, self.flags, self.ids = int(result.frames), int(result.radius), int(result.flags), _copy_struct(result.ids)
        self.tracks, self.v1, self.v2, self.s450 = tracks, v1, v2, s450
        self.offsets = np.arange(-self.radius, self.radius + 1)

    def find(self, value: int) -> list:
        """[(track, offset, 'v1' | 'v2' | 's450')] of every sum equal to `value` (a checksum from a rip database).  An s450
        of a track too short to have one is never a match.  Host only."""
        out = []
        for kind, a in (("v1", self.v1), ("v2", self.v2), ("s450", self.s450)):
            for t, k in zip(*np.nonzero(a == np.uint32(value))):
                if kind == "s450" and self.tracks[t].flags & AR_TRACK_NO_S450:
                    continue
                if kind != "s450" and self.tracks[t].flags & AR_TRACK_SHORT:
                    continue
                out.append((int(t), int(self.offsets[k]), kind))
        return sorted(out)


def ar_ids(track_frames, first=True, last=True, lba0=0) -> ArId:
    """Host only: the disc ids of track lengths in frames (lacx.h); all zero unless the disc is whole (first and last) and
    every track a whole number of 588-frame sectors."""
    n = len(track_frames)
    tf = (C.c_uint64 * max(1, n))(*track_frames)
    out = ArId()
    if lib().lacx_ar_ids(tf, C.c_uint32(n), C.c_uint32((AR_FIRST if first else 0) | (AR_LAST if last else 0)), C.c_uint32(lba0), C.byref(out)) != OK:
        raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
    return out


# ---- bit-compare: offset search and null-test residual (lacx.h) ----
COMPARE_NONE = 2 ** 64 - 1  # LACX_COMPARE_NONE
COMPARE_SIDE_NONE, COMPARE_SIDE_A, COMPARE_SIDE_B = 0, 1, 2
COMPARE_MAX_RADIUS = 32767
COMPARE_ROW_FRAMES = 16384


class ComparePair(C.Structure):
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("centre", C.c_int64), ("radius", C.c_uint32), ("reserved", C.c_uint32)]


class CompareChannelRow(C.Structure):
    """One channel of one row of 16384 domain frames (lacx_compare_channel_row): positions count from the domain's first
    frame, COMPARE_NONE where nothing differs."""
    _fields_ = [("first", C.c_uint64), ("last", C.c_uint64), ("max_at", C.c_uint64), ("sum_abs", C.c_uint64), ("sum_sq", C.c_uint64),
                ("mismatches", C.c_uint32), ("max_abs", C.c_uint32)]


class CompareRow(C.Structure):
    _fields_ = [("ch", CompareChannelRow * 2)]


class CompareChannel(C.Structure):
    _fields_ = [("mismatches", C.c_uint64), ("first", C.c_int64), ("last", C.c_int64), ("peak_at", C.c_int64), ("sum_abs_lo", C.c_uint64),
                ("sum_abs_hi", C.c_uint64), ("sum_sq_lo", C.c_uint64), ("sum_sq_hi", C.c_uint64), ("peak", C.c_uint32), ("reserved", C.c_uint32)]


class Compare(C.Structure):
    """The totals of one pair at its chosen offset (lacx_compare).  Frame positions are on A's axis."""
    _fields_ = [("offset", C.c_int64), ("domain_first", C.c_int64), ("domain_frames", C.c_uint64), ("frames_a", C.c_uint64), ("frames_b", C.c_uint64),
                ("mismatches", C.c_uint64), ("first", C.c_int64), ("last", C.c_int64), ("peak_at", C.c_int64), ("sum_abs_lo", C.c_uint64),
                ("sum_abs_hi", C.c_uint64), ("sum_sq_lo", C.c_uint64), ("sum_sq_hi", C.c_uint64), ("rows", C.c_uint64), ("rows_differ", C.c_uint64),
                ("lead", C.c_uint64), ("tail", C.c_uint64), ("peak", C.c_uint32), ("sample_rate", C.c_uint32), ("peak_channel", C.c_uint8),
                ("channels", C.c_uint8), ("bit_depth", C.c_uint8), ("lead_side", C.c_uint8), ("tail_side", C.c_uint8), ("reserved", C.c_uint8 * 3),
                ("ch", CompareChannel * 2)]

    @property
    def identical(self) -> bool:
        return self.mismatches == 0

    @property
    def sum_abs(self) -> int:
        return self.sum_abs_lo | (self.sum_abs_hi << 64)

    @property
    def sum_sq(self) -> int:
        return self.sum_sq_lo | (self.sum_sq_hi << 64)

    @property
    def peak_dbfs(self) -> float:
        """The residual's peak against full scale of the bit depth; -inf where nothing differs."""
        return 20.0 * math.log10(self.peak / float(1 << (self.bit_depth - 1))) if self.peak else float("-inf")

    @property
    def rms_dbfs(self) -> float:
        """The residual's RMS over every sample of the domain against full scale; -inf where nothing differs."""
        n = self.domain_frames * self.channels
        if not self.sum_sq or not n:
            return float("-inf")
        return 10.0 * math.log10(self.sum_sq / n / float(1 << (self.bit_depth - 1)) ** 2)


class CompareResult:
    """One pair: `totals` (Compare), `rows` (an array of CompareRow), `counts` (uint64 array of mis[] over `offsets`, empty at radius
    0).  Attributes of the totals read through."""

    def __init__(self, totals, rows, counts, centre, radius):
        self.totals, self.rows, self.counts = totals, rows, counts
        self.offsets = np.arange(centre - radius, centre + radius + 1) if len(counts) else np.zeros(0, np.int64)

    def __getattr__(self, name):
        return getattr(self.totals, name)


def compare_combine(rows, channels, bit_depth, sample_rate, frames_a, frames_b, offset=0) -> Compare:
    """Host only: the totals of a pair's rows (lacx_compare_combine)."""
    n = len(rows)
    arr = (CompareRow * max(1, n))(*rows)
    out = Compare()
    if lib().lacx_compare_combine(arr, C.c_uint32(n), C.c_uint8(channels), C.c_uint8(bit_depth), C.c_uint32(sample_rate), C.c_uint64(frames_a),
                                  C.c_uint64(frames_b), C.c_int64(offset), C.byref(out)) != OK:
        raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
    return out


# ---- runs: where a stream is silent, clips or holds one value (lacx.h) ----
RUN_QUIET, RUN_PEAK, RUN_FLAT = 0, 1, 2  # LACX_RUN_*
RUN_ALL = 255
MAX_DETECTORS = 8
RUNS_RERUN = 1
RUN_CHANNELS = {"left": 0, "right": 1, "all": RUN_ALL}


class RunDetector(C.Structure):
    _fields_ = [("kind", C.c_uint8), ("channel", C.c_uint8), ("reserved", C.c_uint8 * 2), ("level", C.c_uint32),
                ("min_frames", C.c_uint64)]


class RunQuery(C.Structure):
    _fields_ = [("first_detector", C.c_uint32), ("detectors", C.c_uint32)]


class Run(C.Structure):
    _fields_ = [("start", C.c_uint64), ("frames", C.c_uint64)]


class RunTotals(C.Structure):
    _fields_ = [("runs", C.c_uint64), ("frames", C.c_uint64), ("longest", C.c_uint64), ("longest_start", C.c_uint64)]


class RunsResult(C.Structure):
    """What a runs call says of an item (lacx_runs_result): the stream's size and losses and per detector the totals."""
    _fields_ = [("frames", C.c_uint64), ("lost_frames", C.c_uint64), ("sample_rate", C.c_uint32), ("blocks", C.c_uint32),
                ("lost_blocks", C.c_uint32), ("flags", C.c_uint32), ("channels", C.c_uint8), ("bit_depth", C.c_uint8),
                ("detectors", C.c_uint8), ("reserved", C.c_uint8 * 5), ("det", RunTotals * MAX_DETECTORS)]

    @property
    def rerun(self) -> bool:
        return bool(self.flags & RUNS_RERUN)


class Detector:
    """A detector as a caller states it, converted per item: level in sample units or dbfs (floor(2^(b-1) * 10^(dB/20))
    at the item's depth b), min_frames or seconds (frames at the item's rate, at least 1)."""

    def __init__(self, kind, level=None, dbfs=None, min_frames=None, seconds=None, channel="all"):
        if level is not None and dbfs is not None:
            raise ValueError("level and dbfs exclude each other")
        if min_frames is not None and seconds is not None:
            raise ValueError("min_frames and seconds exclude each other")
        self.kind, self.level, self.dbfs, self.min_frames, self.seconds = kind, level, dbfs, min_frames, seconds
        self.channel = RUN_CHANNELS[channel] if isinstance(channel, str) else int(channel)

    def resolve(self, bit_depth: int, sample_rate: int) -> RunDetector:
        level = (1 << (bit_depth - 1)) - 1 if self.level == "full" else int(self.level or 0)
        if self.dbfs is not None:
            level = int(math.floor((1 << (bit_depth - 1)) * 10.0 ** (self.dbfs / 20.0)))
        frames = 1 if self.min_frames is None else int(self.min_frames)
        if self.seconds is not None:
            frames = max(1, int(math.floor(self.seconds * sample_rate)))
        return RunDetector(self.kind, self.channel, (C.c_uint8 * 2)(), min(max(level, 0), 0xFFFFFFFF), frames)

    def __repr__(self):
        return f"Detector({('quiet', 'peak', 'flat')[self.kind]}, level={self.level}, dbfs={self.dbfs}, min_frames={self.min_frames}, seconds={self.seconds}, channel={self.channel})"


def quiet(level=None, dbfs=None, min_frames=None, seconds=None, channel="all") -> Detector:
    """Frames with -level <= x <= level in every selected channel (level 0, the default: digital silence)."""
    return Detector(RUN_QUIET, level, dbfs, min_frames, seconds, channel)


def peak(level=None, dbfs=None, min_frames=None, seconds=None, channel="all") -> Detector:
    """Frames with x >= level or x <= -level - 1 in every selected channel; without level or dbfs: full scale, 2^(b-1) - 1."""
    return Detector(RUN_PEAK, "full" if level is None and dbfs is None else level, dbfs, min_frames, seconds, channel)


def flat(min_frames=None, seconds=None, channel="all") -> Detector:
    """Frames whose samples equal the frame before in every selected channel: N equal samples are N - 1 flagged frames."""
    return Detector(RUN_FLAT, 0, None, min_frames, seconds, channel)


class RunList:
    """One detector's answer for one item: `runs`, a [k, 2] uint64 array of (start, frames) ascending by start, and
    `totals` (RunTotals)."""

    def __init__(self, detector: RunDetector, runs: np.ndarray, totals: RunTotals):
        self.detector, self.runs, self.totals = detector, runs, totals

    def __repr__(self):
        return f"RunList(runs={self.totals.runs}, frames={self.totals.frames}, longest={self.totals.longest}@{self.totals.longest_start})"


def sound_pieces(frames: int, quiet_runs, pad: int = 0) -> list:
    """The complement of quiet runs inside [0, frames) as (start, frames) pieces, each widened by `pad` frames on both
    sides, clipped to the stream and merged where pieces touch or overlap.  Pure arithmetic: what split_on_silence cuts."""
    pieces, at = [], 0
    for start, n in list(quiet_runs) + [(frames, 0)]:
        start, n = int(start), int(n)
        if start > at:
            lo, hi = max(0, at - pad), min(frames, start + pad)
            if pieces and lo <= pieces[-1][1]:
                pieces[-1][1] = max(pieces[-1][1], hi)
            else:
                pieces.append([lo, hi])
        at = max(at, start + n)
    return [(lo, hi - lo) for lo, hi in pieces]


def stats_combine(rows, channels: int, bit_depth: int, sample_rate: int = 0) -> Stats:
    """The totals of BlockStats rows (all of an item's, or a sub-range: a window's blocks), as stats_batch makes an item's.
    ValueError for a channel count or depth the library does not know.  Host only."""
    arr = (BlockStats * max(1, len(rows)))(*rows)
    out = Stats()
    if lib().lacx_stats_combine(arr, C.c_uint32(len(rows)), C.c_uint8(channels), C.c_uint8(bit_depth), C.c_uint32(sample_rate), C.byref(out)) != OK:
        raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
    return out


INSPECT_PARTITIONS = 1  # LACX_INSPECT_PARTITIONS (call flag)
BIT_CLASSES = ("header_bits", "tag_bits", "unary_bits", "remainder_bits", "escape_bits", "pad_bits")


class ChannelInfo(C.Structure):
    """How one channel block was coded (lacx_channel_info): predictor, partition order, where its bits and samples go."""
    _fields_ = [("predictor_type", C.c_uint8), ("order", C.c_uint8), ("partition_order", C.c_uint8), ("k_min", C.c_uint8),
                ("k_max", C.c_uint8), ("reserved", C.c_uint8 * 3), ("coef", C.c_int16 * 32),
                ("bits", C.c_uint32), ("header_bits", C.c_uint32), ("tag_bits", C.c_uint32), ("unary_bits", C.c_uint32),
                ("remainder_bits", C.c_uint32), ("escape_bits", C.c_uint32), ("pad_bits", C.c_uint32),
                ("rice_samples", C.c_uint32), ("run_tokens", C.c_uint32), ("run_samples", C.c_uint32),
                ("escape_samples", C.c_uint32), ("bin_samples", C.c_uint32 * 3),
                ("mode_parts", C.c_uint16 * 4), ("mode_samples", C.c_uint16 * 4),
                ("unary_max", C.c_uint32), ("max_u", C.c_uint32), ("sum_u", C.c_uint64)]

    @property
    def partitions(self) -> int:
        return sum(self.mode_parts)


class BlockInfo(C.Structure):
    """One block of an inspected stream (lacx_block_info); a block that does not parse keeps frames, bytes and code."""
    _fields_ = [("frames", C.c_uint32), ("bytes", C.c_uint32), ("code", C.c_uint32), ("ms", C.c_uint8), ("channels", C.c_uint8),
                ("reserved", C.c_uint8 * 2), ("ch", ChannelInfo * 2)]
    # with Decoder.inspect_batch(partitions=True): per channel block [(mode_k, part_bits), ...], else None
    partitions = None


class StreamReport(C.Structure):
    """The totals of an item over the blocks that parse (lacx_stream_report).  Exact integers; `bits_per_sample` and
    `shares` are derived floats and part of no equality."""
    _fields_ = [("frames", C.c_uint64), ("head_bytes", C.c_uint64), ("payload_bytes", C.c_uint64), ("sample_rate", C.c_uint32),
                ("channels", C.c_uint8), ("bit_depth", C.c_uint8), ("stereo_mode", C.c_uint8), ("version", C.c_uint8),
                ("blocks", C.c_uint32), ("lost_blocks", C.c_uint32), ("ms_blocks", C.c_uint32), ("channel_blocks", C.c_uint32),
                ("fixed_blocks", C.c_uint32 * 5), ("fir_blocks", C.c_uint32), ("lpc_blocks", C.c_uint32 * 33),
                ("partition_order_blocks", C.c_uint32 * 9), ("mode_parts", C.c_uint64 * 4), ("mode_samples", C.c_uint64 * 4),
                ("bits", C.c_uint64), ("flag_bits", C.c_uint64), ("header_bits", C.c_uint64), ("tag_bits", C.c_uint64),
                ("unary_bits", C.c_uint64), ("remainder_bits", C.c_uint64), ("escape_bits", C.c_uint64), ("pad_bits", C.c_uint64),
                ("rice_samples", C.c_uint64), ("run_tokens", C.c_uint64), ("run_samples", C.c_uint64),
                ("escape_samples", C.c_uint64), ("bin_samples", C.c_uint64 * 3), ("sum_u_lo", C.c_uint64), ("sum_u_hi", C.c_uint64),
                ("max_u", C.c_uint32), ("unary_max", C.c_uint32), ("k_min", C.c_uint8), ("k_max", C.c_uint8),
                ("reserved", C.c_uint8 * 6)]

    @property
    def sum_u(self) -> int:
        return (self.sum_u_hi << 64) | self.sum_u_lo

    @property
    def samples(self) -> int:
        """The samples of the channel blocks that parse."""
        return sum(self.mode_samples)

    @property
    def bits_per_sample(self) -> float:
        """Derived: payload bits of the blocks that parse per sample of theirs."""
        return 8.0 * self.payload_bytes / self.samples if self.samples else 0.0

    @property
    def shares(self) -> dict:
        """Derived: each bit class (and the per-block flags) as a share of the payload bits of the blocks that parse."""
        total = 8.0 * self.payload_bytes
        return {k: (getattr(self, k) / total if total else 0.0) for k in (*BIT_CLASSES, "flag_bits")}


def inspect_combine(rows, info: "StreamInfo | None" = None) -> StreamReport:
    """The totals of BlockInfo rows (all of an item's, or a sub-range), as inspect_batch makes an item's.  Host only."""
    arr = (BlockInfo * max(1, len(rows)))(*rows)
    out = StreamReport()
    if lib().lacx_inspect_combine(arr, C.c_uint32(len(rows)), C.byref(info) if info is not None else None, C.byref(out)) != OK:
        raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
    return out


# ---- transcode: .lac in, .lac out (lacx_transcode_batch) ----
TO_END = (1 << 64) - 1                       # LACX_TO_END: a segment that runs to its stream's end
CH_KEEP, CH_LEFT, CH_RIGHT, CH_FOLD, CH_SWAP, CH_DUAL = range(6)  # LACX_CH_*
CHANNEL_OPS = {"keep": CH_KEEP, "left": CH_LEFT, "right": CH_RIGHT, "fold": CH_FOLD, "swap": CH_SWAP, "dual": CH_DUAL}
TRANSCODE_VERIFY = 1                         # LACX_TRANSCODE_VERIFY (call flag)


class EditSegment(C.Structure):
    _fields_ = [("lac", C.POINTER(C.c_uint8)), ("size", C.c_uint64), ("start", C.c_uint64), ("frames", C.c_uint64)]


class EditOutput(C.Structure):
    _fields_ = [("first_segment", C.c_uint32), ("segments", C.c_uint32), ("bit_depth", C.c_uint8), ("channel_op", C.c_uint8),
                ("stereo_mode", C.c_uint8), ("reserved", C.c_uint8 * 5)]


class EditResult(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("lac_bytes", C.c_uint64), ("blocks", C.c_uint32), ("data_crc32", C.c_uint32),
                ("sample_rate", C.c_uint32), ("channels", C.c_uint8), ("bit_depth", C.c_uint8), ("verified", C.c_uint8),
                ("reserved", C.c_uint8), ("source_lac_bytes", C.c_uint64)]


# ---- recovery data: the parity sidecar (lacx_recovery_*) ----
REPAIR_TRUNCATED, REPAIR_TRAILING, REPAIR_SIDECAR_TRUNCATED, REPAIR_UNREPAIRED = 1, 2, 4, 8  # LACX_REPAIR_* (result flags)
REPAIR_BEST_EFFORT = 1                                                                       # LACX_REPAIR_BEST_EFFORT (call flag)


class RecoveryParams(C.Structure):
    """The parameters of a recovery sidecar; a zero field means its default (4096, 8, 128)."""
    _fields_ = [("slice_bytes", C.c_uint32), ("parity", C.c_uint16), ("group_data", C.c_uint16)]


class RecoveryInfo(C.Structure):
    """The head of a recovery sidecar; parity_present: the parity records that lie wholly inside it."""
    _fields_ = [("file_bytes", C.c_uint64), ("file_crc32", C.c_uint32), ("slice_bytes", C.c_uint32), ("slices", C.c_uint32),
                ("groups", C.c_uint32), ("parity", C.c_uint16), ("group_data", C.c_uint16), ("parity_present", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class RepairResult(C.Structure):
    """What a recovery scan or repair found: first_bad == slices when no slice is damaged; flags: REPAIR_*."""
    _fields_ = [("file_bytes", C.c_uint64), ("slices", C.c_uint32), ("bad_slices", C.c_uint32), ("repaired_slices", C.c_uint32),
                ("first_bad", C.c_uint32), ("parity_slices", C.c_uint32), ("bad_parity", C.c_uint32), ("worst_group", C.c_uint32),
                ("worst_group_bad", C.c_uint32), ("worst_group_parity", C.c_uint32), ("flags", C.c_uint32)]


def recovery_parse(sidecar: bytes) -> RecoveryInfo:
    """The head of a recovery sidecar; ValueError with the parser's "[recovery-error] ..." text.  Host only."""
    buf = (C.c_uint8 * max(1, len(sidecar))).from_buffer_copy(sidecar if sidecar else b"\0")
    info = RecoveryInfo()
    if lib().lacx_recovery_parse(buf, C.c_uint64(len(sidecar)), C.byref(info)) != OK:
        raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
    return info


def manifest_build(digest: Digest, rows) -> bytes:
    """The manifest (sidecar of block digests) of `digest` and its rows, as digest_blocks_batch / digest_pcm_blocks_batch
    give them.  ValueError where a block is lost or the rows do not fit the digest.  Host only."""
    arr = (BlockDigest * max(1, len(rows)))(*rows)
    out, size = C.POINTER(C.c_uint8)(), C.c_uint64()
    rc = lib().lacx_manifest_build(C.byref(digest), arr, C.c_uint32(len(rows)), C.byref(out), C.byref(size))
    if rc != OK:
        raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
    try:
        return C.string_at(out, size.value)
    finally:
        lib().lacx_free(out)


def manifest_parse(manifest: bytes):
    """(ManifestInfo, [BlockDigest]) of a manifest; ValueError with the parser's "[manifest-error] ..." text.  Host only."""
    buf = (C.c_uint8 * max(1, len(manifest))).from_buffer_copy(manifest if manifest else b"\0")
    cap = max(1, (len(manifest) - 32) // 8) if len(manifest) >= 32 else 1
    info, rows = ManifestInfo(), (BlockDigest * cap)()
    if lib().lacx_manifest_parse(buf, C.c_uint64(len(manifest)), C.byref(info), rows, C.c_uint32(cap)) != OK:
        raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
    return info, [_copy_struct(rows[b]) for b in range(info.blocks)]


def _copy_struct(x):
    out = type(x)()
    C.memmove(C.byref(out), C.byref(x), C.sizeof(x))
    return out


def block_fault_text(code: int) -> str:
    return lib().lacx_block_fault_text(C.c_uint32(code)).decode()


def stream_scan(lac: bytes):
    """The lenient parse of the salvage decode: (StreamInfo, present_blocks, flags), or None when header or block table
    are refused (lacx_decode_last_error has stream_parse's message).  A version-3 file may end early or carry bytes
    behind its last block: present_blocks of its blocks lie whole inside the file.  Host-only."""
    info, present, flags = StreamInfo(), C.c_uint32(), C.c_uint32()
    buf = (C.c_uint8 * max(1, len(lac))).from_buffer_copy(lac if lac else b"\0")
    rc = lib().lacx_stream_scan(buf, C.c_uint64(len(lac)), C.byref(info), C.byref(present), C.byref(flags))
    return (info, int(present.value), int(flags.value)) if rc == OK else None


def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """zlib's crc32_combine: crc32(A + B) from crc32(A), crc32(B) and len(B).  Host only."""
    return int(lib().lacx_crc32_combine(C.c_uint32(crc_a), C.c_uint32(crc_b), C.c_uint64(len_b)))


SAMPLE_I32, SAMPLE_F32 = 0, 1  # LACX_SAMPLE_*


def _sample_type(dtype) -> int:
    """numpy dtype (or its name) -> LACX_SAMPLE_*: int32 or float32 only."""
    dt = np.dtype(dtype)
    if dt == np.int32:
        return SAMPLE_I32
    if dt == np.float32:
        return SAMPLE_F32
    raise ValueError(f"window samples are int32 or float32, not {dt}")


class BatchDecodeError(RuntimeError):
    """Some items of a batch decode failed.  errors: {index: message} (each the message the item's own decode gives);
    results: the call's results with None at the failed indices.  str(): the lowest failing item, "stream i: ..."."""

    def __init__(self, message, errors, results):
        super().__init__(message)
        self.errors = errors
        self.results = results


def stream_parse(lac: bytes):
    """Header + block table of a .lac (ref src/codec/lac/decoder.cpp:90-200); None when inconsistent.  Host-only."""
    info = StreamInfo()
    buf = (C.c_uint8 * max(1, len(lac))).from_buffer_copy(lac if lac else b"\0")
    return info if lib().lacx_stream_parse(buf, C.c_uint64(len(lac)), C.byref(info)) == OK else None


def _scan_in_place(buf: np.ndarray):
    """The StreamInfo of stream_scan of a uint8 array, without copying it; None where it is refused."""
    info, present, flags = StreamInfo(), C.c_uint32(), C.c_uint32()
    rc = lib().lacx_stream_scan(buf.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint64(buf.size), C.byref(info), C.byref(present), C.byref(flags))
    return info if rc == OK else None


def _parse_in_place(buf: np.ndarray):
    """stream_parse of a uint8 array, without copying it."""
    info = StreamInfo()
    rc = lib().lacx_stream_parse(buf.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint64(buf.size), C.byref(info))
    return info if rc == OK else None


def decode(lac: bytes, device: int = -1):
    """LAC::Decoder::decode on the device (ref src/codec/lac/decoder.hpp:10-24): (left, right or None, StreamInfo,
    kernel milliseconds).  Raises RuntimeError("[decode-error] ...") like the reference throws."""
    info = StreamInfo()
    buf = (C.c_uint8 * max(1, len(lac))).from_buffer_copy(lac if lac else b"\0")
    if lib().lacx_stream_parse(buf, C.c_uint64(len(lac)), C.byref(info)) != OK:
        raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
    left = np.empty(info.frames, dtype=np.int32)
    right = np.empty(info.frames, dtype=np.int32) if info.channels == 2 else None
    ms = C.c_float()
    rc = lib().lacx_decode(C.c_int(device), buf, C.c_uint64(len(lac)), left.ctypes.data_as(C.POINTER(C.c_int32)),
                           right.ctypes.data_as(C.POINTER(C.c_int32)) if right is not None else None,
                           C.c_uint64(info.frames), C.byref(ms))
    if rc != OK:
        raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
    return left, right, info, float(ms.value)


class Decoder:
    """Mirror of LAC::Decoder (ref src/codec/lac/decoder.hpp:10-24) over a decoder handle (lacx_decoder_create): the device
    buffers live from call to call, and so do the output arrays when `reuse_output` is set (a fresh numpy array of a few
    hundred MB costs more in first-touch page faults than the decode itself)."""

    def __init__(self, device: int = -1, reuse_output: bool = False):
        h = C.c_void_p()
        if lib().lacx_decoder_create(C.c_int(device), C.byref(h)) != OK:
            raise RuntimeError("lacx_decoder_create failed")
        self._h = h
        self._reuse = reuse_output
        self._left = self._right = None
        self.last_ms = 0.0

    def close(self):
        if self._h is not None:
            lib().lacx_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode(self, lac: bytes):
        """(left, right or None, StreamInfo, kernel milliseconds); RuntimeError("[decode-error] ...") like the reference."""
        info = StreamInfo()
        buf = np.frombuffer(lac, dtype=np.uint8)
        bp = buf.ctypes.data_as(C.POINTER(C.c_uint8))
        if lib().lacx_stream_parse(bp, C.c_uint64(buf.size), C.byref(info)) != OK:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        if self._reuse and self._left is not None and self._left.size == info.frames:
            left, right = self._left, (self._right if info.channels == 2 else None)
        else:
            left = np.empty(info.frames, dtype=np.int32)
            right = np.empty(info.frames, dtype=np.int32) if info.channels == 2 else None
        if right is None and info.channels == 2:
            right = np.empty(info.frames, dtype=np.int32)
        if self._reuse:
            self._left, self._right = left, right
        ms = C.c_float()
        rc = lib().lacx_decoder_decode(self._h, bp, C.c_uint64(buf.size), left.ctypes.data_as(C.POINTER(C.c_int32)),
                                       right.ctypes.data_as(C.POINTER(C.c_int32)) if right is not None else None,
                                       C.c_uint64(info.frames), C.byref(ms))
        if rc != OK:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        return left, right, info, float(ms.value)

    def _decode_wav(self, fn, lac):
        if self._h is None:
            raise RuntimeError("decoder is closed")
        buf = np.frombuffer(lac, dtype=np.uint8)
        out = C.POINTER(C.c_uint8)()
        size = C.c_uint64()
        ms = C.c_float()
        rc = fn(self._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint64(buf.size), C.byref(out), C.byref(size),
                C.byref(ms))
        if rc != OK:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        self.last_ms = float(ms.value)
        return out, size.value

    def decode_wav(self, lac) -> bytes:
        """The .lac as a canonical WAV file image (44-byte header, interleaved PCM, pad byte), byte-identical to the
        reference CLI's `decode` output (ref src/main.cpp:184-431); kernel milliseconds in `last_ms`.
        RuntimeError("[decode-error] ...") like `decode`."""
        out, size = self._decode_wav(lib().lacx_decoder_decode_wav, lac)
        try:
            return C.string_at(out, size)
        finally:
            lib().lacx_free(out)

    def decode_wav_view(self, lac) -> np.ndarray:
        """Zero-copy form of decode_wav: a uint8 view of the decoder's pinned image buffer, valid until this decoder's
        next call (copy it to keep it)."""
        out, size = self._decode_wav(lib().lacx_decoder_decode_wav_view, lac)
        return np.ctypeslib.as_array(out, shape=(size,))


    def _batch(self, n, call):
        """Runs call(item_rc, ms) for a batch of n; returns (rc, {index: message} of the failed items)."""
        if self._h is None:
            raise RuntimeError("decoder is closed")
        rcs = (C.c_int * max(1, n))()
        ms = C.c_float()
        rc = call(rcs, C.byref(ms))
        self.last_ms = float(ms.value)
        if rc == E_INVALID and n == 0:
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        if rc == E_DEVICE:  # the whole call failed
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        errors = {i: lib().lacx_decoder_item_error(self._h, i).decode(errors="replace") for i in range(n) if rcs[i] != OK}
        return rc, errors

    def _wav_batch(self, fn, lacs):
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        spans = (Span * max(1, n))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        outs = (Span * max(1, n))()
        rc, errors = self._batch(n, lambda rcs, ms: fn(self._h, spans, C.c_uint32(n), outs, rcs, ms))
        return rc, errors, outs

    def _raise_batch(self, rc, errors, results):
        if rc != OK:
            raise BatchDecodeError(lib().lacx_decode_last_error().decode(errors="replace"), errors, results)
        return results

    def decode_wav_batch(self, lacs) -> list:
        """Many .lac streams as one device job: the WAV image of each (what decode_wav gives for it alone), kernel
        milliseconds of the batch in `last_ms`.  Failed items raise BatchDecodeError once the others are done."""
        rc, errors, outs = self._wav_batch(lib().lacx_decoder_decode_wav_batch, lacs)
        results = []
        for i in range(len(lacs)):
            o = outs[i]
            if i in errors or not o.data:
                results.append(None)
                continue
            try:
                results.append(C.string_at(o.data, o.size))
            finally:
                lib().lacx_free(o.data)
        return self._raise_batch(rc, errors, results)

    def decode_wav_batch_view(self, lacs) -> list:
        """Zero-copy form of decode_wav_batch: uint8 views of the decoder's pinned image buffer, valid until this
        decoder's next call."""
        rc, errors, outs = self._wav_batch(lib().lacx_decoder_decode_wav_batch_view, lacs)
        results = [None if (i in errors or not outs[i].data) else np.ctypeslib.as_array(outs[i].data, shape=(outs[i].size,))
                   for i in range(len(lacs))]
        return self._raise_batch(rc, errors, results)

    def _faults(self, i) -> list:
        ptr, count = C.POINTER(BlockFault)(), C.c_uint32()
        if lib().lacx_decoder_item_faults(self._h, C.c_uint32(i), C.byref(ptr), C.byref(count)) != OK:
            return []
        out = []
        for k in range(count.value):  # copies: the list dies with the decoder's next call
            f = BlockFault()
            C.memmove(C.byref(f), C.byref(ptr[k]), C.sizeof(BlockFault))
            out.append(f)
        return out

    @staticmethod
    def _copy_result(r) -> SalvageResult:
        out = SalvageResult()
        C.memmove(C.byref(out), C.byref(r), C.sizeof(SalvageResult))
        return out

    @staticmethod
    def _manifest_spans(manifests, n):
        """manifests[i]: bytes, or None (plain salvage for that item) -> (Span array, the buffers that back it)."""
        if len(manifests) != n:
            raise ValueError("one manifest (or None) per stream")
        bufs = [None if m is None else np.frombuffer(m, dtype=np.uint8) for m in manifests]
        spans = (Span * max(1, n))(*[Span(None, 0) if b is None else Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        return spans, bufs

    def salvage_wav(self, lac, manifests=None):
        """Decode through errors: (WAV image bytes, SalvageResult, [BlockFault]).  The image always has the stream's full
        frame count; blocks that do not decode -- or that a truncated file no longer holds -- are silence, listed in the
        fault list.  A clean stream gives decode_wav's bytes and no fault.  RuntimeError only where the container itself
        is refused (stream_parse's message) or the call as a whole fails.
        manifests: the stream's manifest (bytes); a block that decodes to something else is then silence too, code 11."""
        if self._h is None:
            raise RuntimeError("decoder is closed")
        if manifests is not None:
            try:
                return self.salvage_wav_batch([lac], manifests=[manifests])[0]
            except BatchDecodeError as e:
                raise RuntimeError(e.errors[0]) from None
        buf = np.frombuffer(lac, dtype=np.uint8)
        out, size, ms, res = C.POINTER(C.c_uint8)(), C.c_uint64(), C.c_float(), SalvageResult()
        rc = lib().lacx_decoder_salvage_wav(self._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint64(buf.size), C.byref(out),
                                            C.byref(size), C.byref(res), C.byref(ms))
        if rc != OK:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        self.last_ms = float(ms.value)
        try:
            return C.string_at(out, size.value), res, self._faults(0)
        finally:
            lib().lacx_free(out)

    def salvage_wav_batch(self, lacs, manifests=None) -> list:
        """Many streams salvaged as one device job: (WAV image bytes, SalvageResult, [BlockFault]) per item, None for an
        item whose container is refused; those raise BatchDecodeError once the others are done.
        manifests: per item its manifest (bytes) or None; a block whose digest differs is silence, listed with code 11; an
        item whose manifest is refused or does not fit its stream fails."""
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        spans = (Span * max(1, n))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        outs = (Span * max(1, n))()
        res = (SalvageResult * max(1, n))()
        if manifests is not None:
            mspans, _keep = self._manifest_spans(manifests, n)
            rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_salvage_wav_batch_view_checked(
                self._h, spans, mspans, C.c_uint32(n), outs, rcs, res, ms))
        else:
            rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_salvage_wav_batch_view(
                self._h, spans, C.c_uint32(n), outs, rcs, res, ms))
        results = [None if (i in errors or not outs[i].data) else
                   (C.string_at(outs[i].data, outs[i].size), self._copy_result(res[i]), self._faults(i)) for i in range(n)]
        return self._raise_batch(rc, errors, results)

    def salvage_batch_device(self, lacs, outputs, stream: int = 0, manifests=None) -> list:
        """Many streams salvaged into caller-owned device arrays: outputs[i] = (left_ptr, right_ptr or None), int32 arrays
        of stream_scan(lacs[i])[0].frames each on the decoder's device.  Lost blocks are zeros; nothing outside
        [0, frames) is written.  Returns (StreamInfo, SalvageResult, [BlockFault]) per item, None where the container is
        refused; those raise BatchDecodeError once the others are done."""
        if len(outputs) != len(lacs):
            raise ValueError("one output pair per stream")
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        scans = [stream_scan(x) for x in lacs]
        items = (DecodeItem * max(1, n))()
        for it, b, (lp, rp), sc in zip(items, bufs, outputs, scans):
            it.lac = b.ctypes.data_as(C.POINTER(C.c_uint8))
            it.size = b.size
            it.left = lp
            it.right = rp
            it.frames = sc[0].frames if sc is not None else 0
        res = (SalvageResult * max(1, n))()
        if manifests is not None:  # per item its manifest (bytes) or None, as salvage_wav_batch
            mspans, _keep = self._manifest_spans(manifests, n)
            rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_salvage_batch_device_checked(
                self._h, items, mspans, C.c_uint32(n), C.c_void_p(stream), rcs, res, ms))
        else:
            rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_salvage_batch_device(
                self._h, items, C.c_uint32(n), C.c_void_p(stream), rcs, res, ms))
        results = [None if i in errors else (scans[i][0], self._copy_result(res[i]), self._faults(i)) for i in range(n)]
        return self._raise_batch(rc, errors, results)

    def decode_batch_device(self, lacs, outputs, stream: int = 0) -> list:
        """Many .lac streams decoded into caller-owned device arrays: outputs[i] = (left_ptr, right_ptr or None), raw
        device addresses of `frames` int32 each on the decoder's device (a torch tensor's data_ptr()); the work goes on
        `stream` (a raw hipStream_t, 0 = the null stream).  Returns each item's StreamInfo (None where it failed);
        failed items raise BatchDecodeError once the others are done."""
        if len(outputs) != len(lacs):
            raise ValueError("one output pair per stream")
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        infos = [stream_parse(x) for x in lacs]
        items = (DecodeItem * max(1, n))()
        for it, b, (lp, rp), inf in zip(items, bufs, outputs, infos):
            it.lac = b.ctypes.data_as(C.POINTER(C.c_uint8))
            it.size = b.size
            it.left = lp
            it.right = rp
            it.frames = inf.frames if inf is not None else 0
        rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_decode_batch_device(
            self._h, items, C.c_uint32(n), C.c_void_p(stream), rcs, ms))
        results = [None if i in errors else infos[i] for i in range(n)]
        return self._raise_batch(rc, errors, results)

    def decode_window(self, lac, start: int, frames: int, dtype=np.int32):
        """Frames [start, start + frames) of a .lac as (left, right or None) numpy arrays of `dtype` (int32: the integer
        samples; float32: sample * 2^-(bit_depth - 1)).  Only the blocks that overlap the window are decoded (a version-2
        stream decodes in full); kernel milliseconds in `last_ms`.  RuntimeError like `decode`."""
        if self._h is None:
            raise RuntimeError("decoder is closed")
        st = _sample_type(dtype)
        info = StreamInfo()
        buf = np.frombuffer(lac, dtype=np.uint8)
        bp = buf.ctypes.data_as(C.POINTER(C.c_uint8))
        if lib().lacx_stream_parse(bp, C.c_uint64(buf.size), C.byref(info)) != OK:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        n = max(int(frames), 0)
        left = np.empty(n, dtype=np.dtype(dtype))
        right = np.empty(n, dtype=np.dtype(dtype)) if info.channels == 2 else None
        ms = C.c_float()
        rc = lib().lacx_decoder_decode_window(self._h, bp, C.c_uint64(buf.size), C.c_uint64(int(start)),
                                              C.c_uint64(int(frames)), C.c_int(st), C.c_void_p(left.ctypes.data),
                                              C.c_void_p(right.ctypes.data) if right is not None else None, C.byref(ms))
        if rc != OK:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        self.last_ms = float(ms.value)
        return left, right

    def decode_window_batch_device(self, lacs, starts, frames, outputs, dtype="int32", stream: int = 0) -> list:
        """Frame windows of many .lac streams as one device job, into caller-owned device arrays: item i is frames
        [starts[i], starts[i] + frames[i]) of lacs[i] (`frames`: one int for all items or one per item), written to
        outputs[i] = (left_ptr, right_ptr or None), raw device addresses of that many int32 or float32 (`dtype`) on the
        decoder's device, 4-byte aligned (a row of a torch tensor).  The work goes on `stream` (a raw hipStream_t, 0 = the
        null stream).  Returns each item's StreamInfo (None where it failed); failed items raise BatchDecodeError once
        the others are done."""
        st = _sample_type(dtype)
        n = len(lacs)
        counts = [int(frames)] * n if np.ndim(frames) == 0 else [int(f) for f in frames]
        if len(outputs) != n or len(starts) != n or len(counts) != n:
            raise ValueError("one start, frame count and output pair per stream")
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        infos = [_parse_in_place(b) for b in bufs]  # (a window of a long stream: no copy of the stream per item)
        items = (WindowItem * max(1, n))()
        for it, b, s0, f, (lp, rp) in zip(items, bufs, starts, counts, outputs):
            it.lac = b.ctypes.data_as(C.POINTER(C.c_uint8))
            it.size = b.size
            it.start = int(s0)
            it.frames = f
            it.left = lp
            it.right = rp
        rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_decode_window_batch_device(
            self._h, items, C.c_uint32(n), C.c_int(st), C.c_void_p(stream), rcs, ms))
        results = [None if i in errors else infos[i] for i in range(n)]
        return self._raise_batch(rc, errors, results)


    def verify_batch_device(self, lacs, sources, stream: int = 0) -> list:
        """Many .lac streams compared on the device with the PCM they were made from: sources[i] = (data0_ptr,
        data1_ptr or None, layout, channels, frames), device-resident PCM in any PCM_* layout on the decoder's device
        (planar: left and right int32 arrays; interleaved: the WAV data chunk).  The work goes on `stream` (a raw
        hipStream_t, 0 = the null stream); nothing but a few words per item comes back.  Returns each item's VerifyResult
        (all zero: identical).  An item that differs or does not decode raises BatchDecodeError once the others are
        done: errors[i] is its message ("[verify-error] block=N ..." or the decode's own), results[i] its VerifyResult
        where it decoded and differed, None where it failed.  A source may also be a device tensor by itself (pcm_of)."""
        if len(sources) != len(lacs):
            raise ValueError("one source per stream")
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        items = (VerifyItem * max(1, n))()
        for it, b, src in zip(items, bufs, sources):
            it.lac = b.ctypes.data_as(C.POINTER(C.c_uint8))
            it.size = b.size
            if isinstance(src, (tuple, list)):
                d0, d1, layout, channels, frames = src
                it.pcm = Pcm(d0, d1, layout, channels)
            else:  # a tensor, described by itself at the stream's bit depth (see pcm_of)
                info = _parse_in_place(b)  # (a stream that does not parse fails on its own account)
                it.pcm, frames = pcm_of(src, info.bit_depth if info else 16)
            it.frames = frames
        res = (VerifyResult * max(1, n))()
        rcs_seen = []

        def call(rcs, ms):
            rcs_seen.append(rcs)
            return lib().lacx_decoder_verify_batch_device(self._h, items, C.c_uint32(n), C.c_void_p(stream), rcs, res, ms)

        rc, errors = self._batch(n, call)
        rcs = rcs_seen[0]
        results = [res[i] if rcs[i] in (OK, E_MISMATCH) else None for i in range(n)]
        return self._raise_batch(rc, errors, results)

    def digest_batch(self, lacs, stream: int = 0) -> list:
        """Many .lac streams decoded and digested on the device as one job: each item's Digest (CRC-32 of the WAV data
        chunk and of the whole WAV image it decodes to, and its format); only a few bytes per item come back.  The work
        goes on `stream` (a raw hipStream_t, 0 = the null stream); kernel milliseconds in `last_ms`.  An item that does
        not decode raises BatchDecodeError once the others are done (results[i] is None there)."""
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        spans = (Span * max(1, n))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        out = (Digest * max(1, n))()
        rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_digest_batch_device(
            self._h, spans, C.c_uint32(n), C.c_void_p(stream), rcs, out, ms))
        return self._raise_batch(rc, errors, [None if i in errors else out[i] for i in range(n)])

    def digest(self, lac) -> Digest:
        """digest_batch of one stream; RuntimeError with the decode's own message where it does not decode."""
        try:
            return self.digest_batch([lac])[0]
        except BatchDecodeError as e:
            raise RuntimeError(e.errors[0]) from None

    def digest_pcm_batch(self, sources, stream: int = 0) -> list:
        """Device-resident PCM digested where it lies, as one job: sources[i] = (pcm, sample_rate, bit_depth) with pcm a
        device tensor (described by pcm_of at that depth) or a tuple (data0_ptr, data1_ptr or None, layout, channels,
        frames).  Returns each item's Digest: what digest_batch gives for a stream encoded from that source.  An item with
        a sample that is no sample of the depth, or that fails the host's checks, raises BatchDecodeError once the others
        are done."""
        n = len(sources)
        items = (DigestSource * max(1, n))()
        for it, (pcm, rate, depth) in zip(items, sources):
            if isinstance(pcm, (tuple, list)):
                d0, d1, layout, channels, frames = pcm
                it.pcm = Pcm(d0, d1, layout, channels)
            else:
                it.pcm, frames = pcm_of(pcm, depth)
            it.frames, it.sample_rate, it.bit_depth = frames, rate, depth
        out = (Digest * max(1, n))()
        rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_digest_pcm_batch_device(
            self._h, items, C.c_uint32(n), C.c_void_p(stream), rcs, out, ms))
        return self._raise_batch(rc, errors, [None if i in errors else out[i] for i in range(n)])

    def _rows(self, i) -> list:
        ptr, count = C.POINTER(BlockDigest)(), C.c_uint32()
        if lib().lacx_decoder_item_block_digests(self._h, C.c_uint32(i), C.byref(ptr), C.byref(count)) != OK:
            return []
        return [_copy_struct(ptr[k]) for k in range(count.value)]  # copies: the rows die with the decoder's next call

    def digest_blocks_batch(self, lacs, stream: int = 0) -> list:
        """Many streams decoded and digested block by block as one device job, lenient like salvage: per item
        (Digest, [BlockDigest]), None where the container is refused (those raise BatchDecodeError once the others are
        done).  A lost block's row carries its fault code and crc32 0; the Digest's CRCs are those of digest_batch when
        every block decoded, else 0."""
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        spans = (Span * max(1, n))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        out = (Digest * max(1, n))()
        rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_digest_blocks_batch_device(
            self._h, spans, C.c_uint32(n), C.c_void_p(stream), rcs, out, ms))
        return self._raise_batch(rc, errors, [None if i in errors else (_copy_struct(out[i]), self._rows(i)) for i in range(n)])

    def manifest(self, lac) -> bytes:
        """The manifest of what `lac` decodes to; RuntimeError where the container is refused, ValueError where a block
        does not decode."""
        try:
            digest, rows = self.digest_blocks_batch([lac])[0]
        except BatchDecodeError as e:
            raise RuntimeError(e.errors[0]) from None
        return manifest_build(digest, rows)

    def digest_pcm_blocks_batch(self, sources, block_frames: int = 16384, stream: int = 0) -> list:
        """digest_pcm_batch block by block on a regular grid of block_frames frames (256..16384): per item
        (Digest, [BlockDigest]) -- with the encoder's grid of 16384, the rows of the manifest of the .lac made from it."""
        n = len(sources)
        items = (DigestSource * max(1, n))()
        for it, (pcm, rate, depth) in zip(items, sources):
            if isinstance(pcm, (tuple, list)):
                d0, d1, layout, channels, frames = pcm
                it.pcm = Pcm(d0, d1, layout, channels)
            else:
                it.pcm, frames = pcm_of(pcm, depth)
            it.frames, it.sample_rate, it.bit_depth = frames, rate, depth
        out = (Digest * max(1, n))()
        if self._h is None:
            raise RuntimeError("decoder is closed")
        rcs, ms = (C.c_int * max(1, n))(), C.c_float()
        rc = lib().lacx_decoder_digest_pcm_blocks_batch_device(self._h, items, C.c_uint32(n), C.c_uint32(block_frames), C.c_void_p(stream),
                                                               rcs, out, C.byref(ms))
        self.last_ms = float(ms.value)
        if rc == E_INVALID and all(rcs[i] == OK for i in range(n)):  # the call's own arguments
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        if rc == E_DEVICE:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        errors = {i: lib().lacx_decoder_item_error(self._h, i).decode(errors="replace") for i in range(n) if rcs[i] != OK}
        return self._raise_batch(rc, errors, [None if i in errors else (_copy_struct(out[i]), self._rows(i)) for i in range(n)])

    # ---- audio statistics: peaks, energy, silence and bit use ----
    def _stat_rows(self, i) -> list:
        ptr, count = C.POINTER(BlockStats)(), C.c_uint32()
        if lib().lacx_decoder_item_block_stats(self._h, C.c_uint32(i), C.byref(ptr), C.byref(count)) != OK:
            return []
        return [_copy_struct(ptr[k]) for k in range(count.value)]  # copies: the rows die with the decoder's next call

    def stats_batch(self, lacs, stream: int = 0) -> list:
        """Many streams decoded and measured block by block as one device job, lenient like salvage: per item
        (Stats, [BlockStats]), None where the container is refused (those raise BatchDecodeError once the others are
        done).  A lost block's row carries its fault code and is otherwise 0; the totals cover the decoded blocks.  Only
        about 100 bytes per block come back; kernel milliseconds in `last_ms`."""
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        spans = (Span * max(1, n))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        out = (Stats * max(1, n))()
        rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_stats_batch_device(
            self._h, spans, C.c_uint32(n), C.c_void_p(stream), rcs, out, ms))
        return self._raise_batch(rc, errors, [None if i in errors else (_copy_struct(out[i]), self._stat_rows(i)) for i in range(n)])

    def stats(self, lac) -> Stats:
        """The totals of stats_batch of one stream; RuntimeError with the parser's message where the container is refused."""
        try:
            return self.stats_batch([lac])[0][0]
        except BatchDecodeError as e:
            raise RuntimeError(e.errors[0]) from None

    def stats_pcm_batch(self, sources, block_frames: int = 16384, stream: int = 0) -> list:
        """Device-resident PCM measured where it lies on a regular grid of block_frames frames (256..16384): per item
        (Stats, [BlockStats]) -- with the encoder's grid of 16384, what stats_batch gives for the .lac made from it.
        Sources as digest_pcm_blocks_batch takes them: (pcm, sample_rate, bit_depth) with pcm a device tensor or a tuple
        (data0_ptr, data1_ptr or None, layout, channels, frames)."""
        n = len(sources)
        items = (DigestSource * max(1, n))()
        for it, (pcm, rate, depth) in zip(items, sources):
            if isinstance(pcm, (tuple, list)):
                d0, d1, layout, channels, frames = pcm
                it.pcm = Pcm(d0, d1, layout, channels)
            else:
                it.pcm, frames = pcm_of(pcm, depth)
            it.frames, it.sample_rate, it.bit_depth = frames, rate, depth
        out = (Stats * max(1, n))()
        if self._h is None:
            raise RuntimeError("decoder is closed")
        rcs, ms = (C.c_int * max(1, n))(), C.c_float()
        rc = lib().lacx_decoder_stats_pcm_batch_device(self._h, items, C.c_uint32(n), C.c_uint32(block_frames), C.c_void_p(stream),
                                                       rcs, out, C.byref(ms))
        self.last_ms = float(ms.value)
        if rc == E_INVALID and all(rcs[i] == OK for i in range(n)):  # the call's own arguments
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        if rc == E_DEVICE:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        errors = {i: lib().lacx_decoder_item_error(self._h, i).decode(errors="replace") for i in range(n) if rcs[i] != OK}
        return self._raise_batch(rc, errors, [None if i in errors else (_copy_struct(out[i]), self._stat_rows(i)) for i in range(n)])

    # ---- loudness: BS.1770 integrated, momentary, short-term and range ----
    def _loud_rows(self, i):
        ptr, count = C.POINTER(LoudnessRow)(), C.c_uint32()
        if lib().lacx_decoder_item_loudness_rows(self._h, C.c_uint32(i), C.byref(ptr), C.byref(count)) != OK:
            count.value = 0
        rows = (LoudnessRow * count.value)()  # one copy: the rows die with the decoder's next call (a song has thousands)
        if count.value:
            C.memmove(rows, ptr, C.sizeof(rows))
        return rows

    def loudness_batch(self, lacs, stream: int = 0) -> list:
        """Many streams decoded and measured after ITU-R BS.1770 as one device job, strict like digest_batch: per item
        (Loudness, a ctypes array of LoudnessRow), None where the stream does not parse or decode (those raise BatchDecodeError once the
        others are done).  One row per sub-block of sample_rate / 10 frames comes back, not the PCM; kernel milliseconds
        in `last_ms`.  Nothing is applied to the audio."""
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        spans = (Span * max(1, n))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        out = (Loudness * max(1, n))()
        rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_loudness_batch_device(
            self._h, spans, C.c_uint32(n), C.c_void_p(stream), rcs, out, ms))
        return self._raise_batch(rc, errors, [None if i in errors else (_copy_struct(out[i]), self._loud_rows(i)) for i in range(n)])

    def loudness(self, lac) -> Loudness:
        """The totals of loudness_batch of one stream; RuntimeError with the decode's message where it fails."""
        try:
            return self.loudness_batch([lac])[0][0]
        except BatchDecodeError as e:
            raise RuntimeError(e.errors[0]) from None

    def loudness_pcm_batch(self, sources, stream: int = 0) -> list:
        """Device-resident PCM measured where it lies: per item (Loudness, [LoudnessRow]) -- what loudness_batch gives for
        the .lac made from it.  Sources as digest_pcm_blocks_batch takes them: (pcm, sample_rate, bit_depth) with pcm a
        device tensor or a tuple (data0_ptr, data1_ptr or None, layout, channels, frames)."""
        n = len(sources)
        items = (DigestSource * max(1, n))()
        for it, (pcm, rate, depth) in zip(items, sources):
            if isinstance(pcm, (tuple, list)):
                d0, d1, layout, channels, frames = pcm
                it.pcm = Pcm(d0, d1, layout, channels)
            else:
                it.pcm, frames = pcm_of(pcm, depth)
            it.frames, it.sample_rate, it.bit_depth = frames, rate, depth
        out = (Loudness * max(1, n))()
        if self._h is None:
            raise RuntimeError("decoder is closed")
        rcs, ms = (C.c_int * max(1, n))(), C.c_float()
        rc = lib().lacx_decoder_loudness_pcm_batch_device(self._h, items, C.c_uint32(n), C.c_void_p(stream), rcs, out, C.byref(ms))
        self.last_ms = float(ms.value)
        if rc == E_INVALID and all(rcs[i] == OK for i in range(n)):  # the call's own arguments
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        if rc == E_DEVICE:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        errors = {i: lib().lacx_decoder_item_error(self._h, i).decode(errors="replace") for i in range(n) if rcs[i] != OK}
        return self._raise_batch(rc, errors, [None if i in errors else (_copy_struct(out[i]), self._loud_rows(i)) for i in range(n)])

    # ---- true peak: the BS.1770 maximum of the 4x oversampled signal ----
    def _peak_rows(self, i):
        ptr, count = C.POINTER(TruePeakRow)(), C.c_uint32()
        if lib().lacx_decoder_item_truepeak_rows(self._h, C.c_uint32(i), C.byref(ptr), C.byref(count)) != OK:
            count.value = 0
        rows = (TruePeakRow * count.value)()  # one copy: the rows die with the decoder's next call
        if count.value:
            C.memmove(rows, ptr, C.sizeof(rows))
        return rows

    def truepeak_batch(self, lacs, stream: int = 0) -> list:
        """Many streams decoded and their true peak (ITU-R BS.1770 Annex 2) taken as one device job, strict like digest_batch:
        per item (TruePeak, a ctypes array of TruePeakRow), None where the stream does not parse or decode (those raise
        BatchDecodeError once the others are done).  One row per 16384 frames comes back, not the PCM; kernel milliseconds in
        `last_ms`.  Nothing is applied to the audio."""
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        spans = (Span * max(1, n))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        out = (TruePeak * max(1, n))()
        rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_truepeak_batch_device(
            self._h, spans, C.c_uint32(n), C.c_void_p(stream), rcs, out, ms))
        return self._raise_batch(rc, errors, [None if i in errors else (_copy_struct(out[i]), self._peak_rows(i)) for i in range(n)])

    def truepeak(self, lac) -> TruePeak:
        """The totals of truepeak_batch of one stream; RuntimeError with the decode's message where it fails."""
        try:
            return self.truepeak_batch([lac])[0][0]
        except BatchDecodeError as e:
            raise RuntimeError(e.errors[0]) from None

    def truepeak_pcm_batch(self, sources, stream: int = 0) -> list:
        """Device-resident PCM measured where it lies: per item (TruePeak, [TruePeakRow]) -- what truepeak_batch gives for the
        .lac made from it.  Sources as loudness_pcm_batch takes them."""
        n = len(sources)
        items = (DigestSource * max(1, n))()
        for it, (pcm, rate, depth) in zip(items, sources):
            if isinstance(pcm, (tuple, list)):
                d0, d1, layout, channels, frames = pcm
                it.pcm = Pcm(d0, d1, layout, channels)
            else:
                it.pcm, frames = pcm_of(pcm, depth)
            it.frames, it.sample_rate, it.bit_depth = frames, rate, depth
        out = (TruePeak * max(1, n))()
        if self._h is None:
            raise RuntimeError("decoder is closed")
        rcs, ms = (C.c_int * max(1, n))(), C.c_float()
        rc = lib().lacx_decoder_truepeak_pcm_batch_device(self._h, items, C.c_uint32(n), C.c_void_p(stream), rcs, out, C.byref(ms))
        self.last_ms = float(ms.value)
        if rc == E_INVALID and all(rcs[i] == OK for i in range(n)):  # the call's own arguments
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        if rc == E_DEVICE:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        errors = {i: lib().lacx_decoder_item_error(self._h, i).decode(errors="replace") for i in range(n) if rcs[i] != OK}
        return self._raise_batch(rc, errors, [None if i in errors else (_copy_struct(out[i]), self._peak_rows(i)) for i in range(n)])

    # ---- spectrum: the long-term power spectrum in 64 bands and the bandwidth ----
    def _spec_rows(self, i):
        ptr, count = C.POINTER(SpectrumRow)(), C.c_uint32()
        if lib().lacx_decoder_item_spectrum_rows(self._h, C.c_uint32(i), C.byref(ptr), C.byref(count)) != OK:
            count.value = 0
        rows = (SpectrumRow * count.value)()  # one copy: the rows die with the decoder's next call
        if count.value:
            C.memmove(rows, ptr, C.sizeof(rows))
        return rows

    def spectrum_batch(self, lacs, window: int = 2048, floor_db: float = -100.0, stream: int = 0) -> list:
        """Many streams decoded and their banded power spectrum (Hann windows of `window` frames, hop window / 2, FP64) taken
        as one device job, strict like digest_batch: per item (Spectrum, a ctypes array of SpectrumRow), None where the stream
        does not parse or decode (those raise BatchDecodeError once the others are done).  One row per 16384 frames comes
        back, not the PCM; kernel milliseconds in `last_ms`.  ValueError for a window that is none of SPECTRUM_WINDOWS."""
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        spans = (Span * max(1, n))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        out = (Spectrum * max(1, n))()
        rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_spectrum_batch_device(
            self._h, spans, C.c_uint32(n), C.c_uint32(window), C.c_double(floor_db), C.c_void_p(stream), rcs, out, ms))
        if rc == E_INVALID and not errors:  # the call's own arguments: the window
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        return self._raise_batch(rc, errors, [None if i in errors else (_copy_struct(out[i]), self._spec_rows(i)) for i in range(n)])

    def spectrum(self, lac, window: int = 2048, floor_db: float = -100.0) -> Spectrum:
        """The totals of spectrum_batch of one stream; RuntimeError with the decode's message where it fails."""
        try:
            return self.spectrum_batch([lac], window, floor_db)[0][0]
        except BatchDecodeError as e:
            raise RuntimeError(e.errors[0]) from None

    def spectrum_pcm_batch(self, sources, window: int = 2048, floor_db: float = -100.0, stream: int = 0) -> list:
        """Device-resident PCM measured where it lies: per item (Spectrum, [SpectrumRow]) -- what spectrum_batch gives for the
        .lac made from it.  Sources as truepeak_pcm_batch takes them."""
        n = len(sources)
        items = (DigestSource * max(1, n))()
        for it, (pcm, rate, depth) in zip(items, sources):
            if isinstance(pcm, (tuple, list)):
                d0, d1, layout, channels, frames = pcm
                it.pcm = Pcm(d0, d1, layout, channels)
            else:
                it.pcm, frames = pcm_of(pcm, depth)
            it.frames, it.sample_rate, it.bit_depth = frames, rate, depth
        out = (Spectrum * max(1, n))()
        if self._h is None:
            raise RuntimeError("decoder is closed")
        rcs, ms = (C.c_int * max(1, n))(), C.c_float()
        rc = lib().lacx_decoder_spectrum_pcm_batch_device(self._h, items, C.c_uint32(n), C.c_uint32(window), C.c_double(floor_db), C.c_void_p(stream),
                                                          rcs, out, C.byref(ms))
        self.last_ms = float(ms.value)
        if rc == E_INVALID and all(rcs[i] == OK for i in range(n)):  # the call's own arguments
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        if rc == E_DEVICE:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        errors = {i: lib().lacx_decoder_item_error(self._h, i).decode(errors="replace") for i in range(n) if rcs[i] != OK}
        return self._raise_batch(rc, errors, [None if i in errors else (_copy_struct(out[i]), self._spec_rows(i)) for i in range(n)])

    # ---- rip checksums: AccurateRip v1 / v2 at every read offset ----
    @staticmethod
    def _ar_discs(discs):
        """[(sources, tracks or None, radius, first, last, lba0)] -> the flat source list, track_frames, ArDisc array."""
        flat, tf = [], []
        recs = (ArDisc * max(1, len(discs)))()
        for rec, d in zip(recs, discs):
            sources, tracks, radius, first, last, lba0 = (tuple(d) + (None, 0, True, True, 0)[len(d) - 1:])[:6]
            rec.first_source, rec.sources = len(flat), len(sources)
            rec.first_track, rec.tracks = len(tf), len(tracks) if tracks is not None else 0
            rec.flags, rec.radius, rec.lba0 = (AR_FIRST if first else 0) | (AR_LAST if last else 0), radius, lba0
            flat += list(sources)
            tf += list(tracks) if tracks is not None else []
        return flat, (C.c_uint64 * max(1, len(tf)))(*tf), len(tf), recs

    def _ar_finish(self, n, rc, rcs, out):
        if rc == E_DEVICE:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        errors = {k: lib().lacx_decoder_item_error(self._h, k).decode(errors="replace") for k in range(n) if rcs[k] != OK}
        results = []
        for k in range(n):
            if k in errors:
                results.append(None)
                continue
            ptr, count = C.POINTER(ArTrack)(), C.c_uint32()
            assert lib().lacx_decoder_item_ar_tracks(self._h, C.c_uint32(k), C.byref(ptr), C.byref(count)) == OK
            tracks = [_copy_struct(ptr[t]) for t in range(count.value)]
            width = 2 * out[k].radius + 1
            sums = np.zeros((3, count.value, width), np.uint32)
            for t in range(count.value):
                p = [C.POINTER(C.c_uint32)() for _ in range(3)]
                w = C.c_uint32()
                assert lib().lacx_decoder_item_ar_sums(self._h, C.c_uint32(k), C.c_uint32(t), C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(w)) == OK
                for q in range(3):  # one copy: the sums die with the decoder's next call
                    sums[q, t] = np.ctypeslib.as_array(p[q], shape=(w.value,))
            results.append(AccurateRip(out[k], tracks, sums[0], sums[1], sums[2]))
        if rc != OK:
            e = BatchDecodeError(lib().lacx_decode_last_error().decode(errors="replace"), errors, results)
            e.codes = {k: int(rcs[k]) for k in errors}
            raise e
        return results

    def accuraterip_batch(self, discs, stream: int = 0) -> list:
        """Many discs of CD audio (2 channels, 16 bit, 44100 Hz) decoded and their AccurateRip v1 / v2 track checksums and
        450th-sector sums taken at every read offset within a radius, as one device job, strict like digest_batch.  discs:
        [(lacs, tracks=None, radius=0, first=True, last=True, lba0=0)] -- the streams that together are the disc, in order;
        the track lengths in frames (None: one track per stream); the radius in frames, at most 2939.  Per disc an
        AccurateRip, None where it is refused or one of its streams does not decode (those raise BatchDecodeError once the
        others are done).  Kernel milliseconds in `last_ms`."""
        if self._h is None:
            raise RuntimeError("decoder is closed")
        flat, tf, ntf, recs = self._ar_discs(discs)
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in flat]
        spans = (Span * max(1, len(bufs)))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        n = len(discs)
        out, rcs, ms = (ArResult * max(1, n))(), (C.c_int * max(1, n))(), C.c_float()
        rc = lib().lacx_decoder_accuraterip_batch_device(self._h, spans, C.c_uint32(len(bufs)), tf, C.c_uint32(ntf), recs, C.c_uint32(n), C.c_void_p(stream),
                                                         rcs, out, C.byref(ms))
        self.last_ms = float(ms.value)
        if rc == E_INVALID and all(rcs[k] == OK for k in range(n)):  # the call's own arguments
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        return self._ar_finish(n, rc, rcs, out)

    def accuraterip(self, lacs, tracks=None, radius: int = 0, first: bool = True, last: bool = True, lba0: int = 0) -> AccurateRip:
        """accuraterip_batch of one disc; ValueError where the disc is refused, RuntimeError where a stream does not decode."""
        try:
            return self.accuraterip_batch([(lacs, tracks, radius, first, last, lba0)])[0]
        except BatchDecodeError as e:
            raise (ValueError if e.codes[0] == E_INVALID else RuntimeError)(e.errors[0]) from None

    def accuraterip_pcm_batch(self, discs, stream: int = 0) -> list:
        """Device-resident PCM checked where it lies: discs as accuraterip_batch takes them, with sources as
        truepeak_pcm_batch takes them in the place of streams -- what accuraterip_batch gives for the .lac files made from
        them."""
        if self._h is None:
            raise RuntimeError("decoder is closed")
        flat, tf, ntf, recs = self._ar_discs(discs)
        items = (DigestSource * max(1, len(flat)))()
        for it, (pcm, rate, depth) in zip(items, flat):
            if isinstance(pcm, (tuple, list)):
                d0, d1, layout, channels, frames = pcm
                it.pcm = Pcm(d0, d1, layout, channels)
            else:
                it.pcm, frames = pcm_of(pcm, depth)
            it.frames, it.sample_rate, it.bit_depth = frames, rate, depth
        n = len(discs)
        out, rcs, ms = (ArResult * max(1, n))(), (C.c_int * max(1, n))(), C.c_float()
        rc = lib().lacx_decoder_accuraterip_pcm_batch_device(self._h, items, C.c_uint32(len(flat)), tf, C.c_uint32(ntf), recs, C.c_uint32(n),
                                                             C.c_void_p(stream), rcs, out, C.byref(ms))
        self.last_ms = float(ms.value)
        if rc == E_INVALID and all(rcs[k] == OK for k in range(n)):
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        return self._ar_finish(n, rc, rcs, out)

    # ---- bit-compare: offset search and null-test residual ----
    @staticmethod
    def _compare_pairs(pairs):
        recs = (ComparePair * max(1, len(pairs)))()
        for rec, p in zip(recs, pairs):
            a, b, centre, radius = (tuple(p) + (0, 0))[:4]
            if not (0 <= a < 2 ** 32 and 0 <= b < 2 ** 32 and -2 ** 63 <= centre < 2 ** 63 and 0 <= radius < 2 ** 32):
                raise ValueError("pair out of the ABI's range: %r" % (p,))
            rec.a, rec.b, rec.centre, rec.radius = a, b, centre, radius
        return recs

    def _compare_finish(self, recs, n, rc, rcs, out):
        if rc == E_DEVICE:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        errors = {k: lib().lacx_decoder_item_error(self._h, k).decode(errors="replace") for k in range(n) if rcs[k] != OK}
        results = []
        for k in range(n):
            if k in errors:
                results.append(None)
                continue
            ptr, count = C.POINTER(CompareRow)(), C.c_uint32()
            assert lib().lacx_decoder_item_compare_rows(self._h, C.c_uint32(k), C.byref(ptr), C.byref(count)) == OK
            rows = (CompareRow * count.value).from_buffer_copy(C.string_at(ptr, C.sizeof(CompareRow) * count.value))  # one copy: they die with the next call
            cp, cn = C.POINTER(C.c_uint64)(), C.c_uint32()
            assert lib().lacx_decoder_item_compare_counts(self._h, C.c_uint32(k), C.byref(cp), C.byref(cn)) == OK
            counts = np.array(np.ctypeslib.as_array(cp, shape=(cn.value,)), np.uint64) if cn.value else np.zeros(0, np.uint64)
            results.append(CompareResult(_copy_struct(out[k]), rows, counts, int(recs[k].centre), int(recs[k].radius)))
        if rc != OK:
            e = BatchDecodeError(lib().lacx_decode_last_error().decode(errors="replace"), errors, results)
            e.codes = {k: int(rcs[k]) for k in errors}
            raise e
        return results

    def compare_batch(self, lacs, pairs, stream: int = 0) -> list:
        """Many .lac streams decoded and compared in pairs as one device job, strict like digest_batch.  pairs: [(a, b,
        centre=0, radius=0)] -- two indices into `lacs` (one stream may stand in many pairs and is decoded once), and the
        offsets centre - radius .. centre + radius of b against a to search (radius at most 32767).  Per pair a
        CompareResult at the offset with the fewest mismatches, None where the pair is refused or one of its streams does
        not decode (those raise BatchDecodeError once the others are done).  Kernel milliseconds in `last_ms`."""
        if self._h is None:
            raise RuntimeError("decoder is closed")
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        spans = (Span * max(1, len(bufs)))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        recs, n = self._compare_pairs(pairs), len(pairs)
        out, rcs, ms = (Compare * max(1, n))(), (C.c_int * max(1, n))(), C.c_float()
        rc = lib().lacx_decoder_compare_batch_device(self._h, spans, C.c_uint32(len(bufs)), recs, C.c_uint32(n), C.c_void_p(stream), rcs, out, C.byref(ms))
        self.last_ms = float(ms.value)
        if rc == E_INVALID and all(rcs[k] == OK for k in range(n)):  # the call's own arguments
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        return self._compare_finish(recs, n, rc, rcs, out)

    def compare(self, a, b, centre: int = 0, radius: int = 0) -> CompareResult:
        """compare_batch of one pair of .lac streams; ValueError where the pair is refused, RuntimeError where a stream does
        not decode."""
        try:
            return self.compare_batch([a, b], [(0, 1, centre, radius)])[0]
        except BatchDecodeError as e:
            raise (ValueError if e.codes[0] == E_INVALID else RuntimeError)(e.errors[0]) from None

    def compare_pcm_batch(self, sources, pairs, stream: int = 0) -> list:
        """Device-resident PCM compared where it lies: sources as truepeak_pcm_batch takes them, pairs as compare_batch --
        what compare_batch gives for the .lac files made from them."""
        if self._h is None:
            raise RuntimeError("decoder is closed")
        items = (DigestSource * max(1, len(sources)))()
        for it, (pcm, rate, depth) in zip(items, sources):
            if isinstance(pcm, (tuple, list)):
                d0, d1, layout, channels, frames = pcm
                it.pcm = Pcm(d0, d1, layout, channels)
            else:
                it.pcm, frames = pcm_of(pcm, depth)
            it.frames, it.sample_rate, it.bit_depth = frames, rate, depth
        recs, n = self._compare_pairs(pairs), len(pairs)
        out, rcs, ms = (Compare * max(1, n))(), (C.c_int * max(1, n))(), C.c_float()
        rc = lib().lacx_decoder_compare_pcm_batch_device(self._h, items, C.c_uint32(len(sources)), recs, C.c_uint32(n), C.c_void_p(stream), rcs, out,
                                                         C.byref(ms))
        self.last_ms = float(ms.value)
        if rc == E_INVALID and all(rcs[k] == OK for k in range(n)):
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        return self._compare_finish(recs, n, rc, rcs, out)

    # ---- runs: where a stream is silent, clips or holds one value ----
    @staticmethod
    def _detector_tables(detectors, n, formats):
        """detectors: one list for all items or one list per item (of Detector or RunDetector); formats[i]: (bit_depth,
        sample_rate) or None.  -> (RunQuery array, RunDetector array, count, per item the resolved detectors)."""
        per_item = n > 0 and len(detectors) == n and all(isinstance(x, (list, tuple)) for x in detectors)
        flat_list, queries, resolved = [], (RunQuery * max(1, n))(), []
        for i in range(n):
            depth, rate = formats[i] or (16, 1)
            mine = [d.resolve(depth, rate) if isinstance(d, Detector) else d for d in (detectors[i] if per_item else detectors)]
            queries[i] = RunQuery(len(flat_list), len(mine))
            flat_list.extend(mine)
            resolved.append(mine)
        return queries, (RunDetector * max(1, len(flat_list)))(*flat_list), len(flat_list), resolved

    def _run_lists(self, i, resolved, res) -> list:
        out = []
        for k, det in enumerate(resolved):
            ptr, count = C.POINTER(Run)(), C.c_uint64()
            if lib().lacx_decoder_item_runs(self._h, C.c_uint32(i), C.c_uint32(k), C.byref(ptr), C.byref(count)) != OK:
                raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
            runs = np.zeros((count.value, 2), dtype=np.uint64)  # a copy: the lists die with the decoder's next call
            if count.value:
                C.memmove(runs.ctypes.data, ptr, 16 * count.value)
            out.append(RunList(det, runs, _copy_struct(res.det[k])))
        return out

    def runs_batch(self, lacs, detectors, stream: int = 0) -> list:
        """Many streams decoded and searched for runs as one device job, lenient like stats_batch: per item
        (RunsResult, [RunList per detector]), None where the container or the item's detectors are refused (those raise
        BatchDecodeError once the others are done).  detectors: one list for all items or one list per item, of
        lacx.quiet / peak / flat (converted at each item's depth and rate) or RunDetector records.  Every list is complete
        and ascending by start; a lost block splits a run.  Kernel milliseconds in `last_ms`."""
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        spans = (Span * max(1, n))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        formats = []
        for b in bufs:
            info = _scan_in_place(b)  # (the format: what the detectors' dBFS and seconds refer to)
            formats.append((info.bit_depth, info.sample_rate) if info else None)
        queries, dets, ndets, resolved = self._detector_tables(detectors, n, formats)
        out = (RunsResult * max(1, n))()
        if n and ndets == 0:
            raise ValueError("no detectors")
        rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_runs_batch_device(
            self._h, spans, queries, C.c_uint32(n), dets, C.c_uint32(ndets), C.c_void_p(stream), rcs, out, ms))
        if rc == E_INVALID and not errors:
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        return self._raise_batch(rc, errors, [None if i in errors else (_copy_struct(out[i]), self._run_lists(i, resolved[i], out[i])) for i in range(n)])

    def runs(self, lac, detectors) -> list:
        """The [RunList per detector] of runs_batch of one stream; RuntimeError with the item's message where it is refused."""
        try:
            return self.runs_batch([lac], list(detectors))[0][1]
        except BatchDecodeError as e:
            raise RuntimeError(e.errors[0]) from None

    def runs_pcm_batch(self, sources, detectors, stream: int = 0) -> list:
        """Device-resident PCM searched for runs where it lies: per item (RunsResult, [RunList per detector]) -- what
        runs_batch gives for the .lac made from it.  Sources as stats_pcm_batch takes them."""
        n = len(sources)
        items = (DigestSource * max(1, n))()
        formats = []
        for it, (pcm, rate, depth) in zip(items, sources):
            if isinstance(pcm, (tuple, list)):
                d0, d1, layout, channels, frames = pcm
                it.pcm = Pcm(d0, d1, layout, channels)
            else:
                it.pcm, frames = pcm_of(pcm, depth)
            it.frames, it.sample_rate, it.bit_depth = frames, rate, depth
            formats.append((depth if depth in (16, 24) else 16, rate))
        queries, dets, ndets, resolved = self._detector_tables(detectors, n, formats)
        out = (RunsResult * max(1, n))()
        if self._h is None:
            raise RuntimeError("decoder is closed")
        rcs, ms = (C.c_int * max(1, n))(), C.c_float()
        rc = lib().lacx_decoder_runs_pcm_batch_device(self._h, items, queries, C.c_uint32(n), dets, C.c_uint32(ndets), C.c_void_p(stream),
                                                      rcs, out, C.byref(ms))
        self.last_ms = float(ms.value)
        if rc == E_INVALID and all(rcs[i] == OK for i in range(n)):  # the call's own arguments
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        if rc == E_DEVICE:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        errors = {i: lib().lacx_decoder_item_error(self._h, i).decode(errors="replace") for i in range(n) if rcs[i] != OK}
        return self._raise_batch(rc, errors, [None if i in errors else (_copy_struct(out[i]), self._run_lists(i, resolved[i], out[i])) for i in range(n)])

    def _sound_pieces(self, lac, level, min_frames, pad):
        try:
            res, lists = self.runs_batch([lac], [RunDetector(RUN_QUIET, RUN_ALL, (C.c_uint8 * 2)(), int(level), int(min_frames))])[0]
        except BatchDecodeError as e:
            raise RuntimeError(e.errors[0]) from None
        if res.lost_blocks:
            raise ValueError(f"stream has {res.lost_blocks} lost blocks: silence cannot be told from loss")
        return sound_pieces(int(res.frames), lists[0].runs.tolist(), int(pad))

    def split_on_silence(self, encoder: "Encoder", lac, level: int, min_frames: int, pad: int = 0, verify: bool = False) -> list:
        """The stream cut at its silences: one QUIET detector over all channels (|x| <= level for min_frames frames at
        least), the sounding pieces between its runs widened by `pad` frames, clipped and merged, then one transcode_batch
        with one output per piece.  Returns [(start, frames, bytes)]: every output is byte for byte what `cut` gives for
        that range.  A stream with a lost block is refused (ValueError); one that is all silence gives no outputs."""
        pieces = self._sound_pieces(lac, level, min_frames, pad)
        if not pieces:
            return []
        outs = self.transcode_batch(encoder, [([(lac, start, n)],) for start, n in pieces], verify)
        return [(start, n, data) for (start, n), (data, _res) in zip(pieces, outs)]

    def trim_silence(self, encoder: "Encoder", lac, level: int, min_frames: int, pad: int = 0, verify: bool = False):
        """The stream without its leading and trailing silence: from the first sounding piece's start to the last one's
        end, as (start, frames, bytes); None where the stream is all silence."""
        pieces = self._sound_pieces(lac, level, min_frames, pad)
        if not pieces:
            return None
        start, end = pieces[0][0], pieces[-1][0] + pieces[-1][1]
        return start, end - start, self.cut(encoder, lac, start, end - start, verify)

    # ---- stream inspection: predictors, modes, bit budget ----
    def _info_rows(self, i, partitions) -> list:
        ptr, count = C.POINTER(BlockInfo)(), C.c_uint32()
        if lib().lacx_decoder_item_block_info(self._h, C.c_uint32(i), C.byref(ptr), C.byref(count)) != OK:
            return []
        rows = [_copy_struct(ptr[k]) for k in range(count.value)]  # copies: the rows die with the decoder's next call
        for b, row in enumerate(rows if partitions else ()):
            row.partitions = []
            for c in range(row.channels):
                mk, pb, n = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint32)(), C.c_uint32()
                if lib().lacx_decoder_item_partitions(self._h, C.c_uint32(i), C.c_uint32(b), C.c_uint32(c), C.byref(mk), C.byref(pb), C.byref(n)) != OK:
                    raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
                row.partitions.append([(int(mk[p]), int(pb[p])) for p in range(n.value)])
        return rows

    def inspect_batch(self, lacs, partitions: bool = False, stream: int = 0) -> list:
        """Many streams walked token by token as one device job -- no synthesis, no PCM -- lenient like stats_batch: per
        item (StreamReport, [BlockInfo]), None where the container is refused (those raise BatchDecodeError once the others
        are done).  A block that does not parse carries its code and is otherwise 0; the totals cover the blocks that
        parse.  Codes 5 and 7 need samples and are never reported here.  partitions: every row's `partitions` holds per
        channel block the (mode_k, part_bits) of its partitions.  Kernel milliseconds in `last_ms`."""
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        spans = (Span * max(1, n))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        out = (StreamReport * max(1, n))()
        rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_decoder_inspect_batch_device(
            self._h, spans, C.c_uint32(n), C.c_uint32(INSPECT_PARTITIONS if partitions else 0), C.c_void_p(stream), rcs, out, ms))
        return self._raise_batch(rc, errors, [None if i in errors else (_copy_struct(out[i]), self._info_rows(i, partitions)) for i in range(n)])

    def inspect_guard(self):
        """(guarded, changed): with LACX_INSPECT_GUARD=1 in the environment, the guard bytes behind the last inspection job's
        tables on the device and how many of them the job changed (lacx_decoder_inspect_guard); (0, 0) without."""
        guarded, changed = C.c_uint64(), C.c_uint64()
        if lib().lacx_decoder_inspect_guard(self._h, C.byref(guarded), C.byref(changed)) != OK:
            raise RuntimeError(lib().lacx_decode_last_error().decode(errors="replace"))
        return guarded.value, changed.value

    def inspect(self, lac) -> StreamReport:
        """The totals of inspect_batch of one stream; RuntimeError with the parser's message where the container is refused."""
        try:
            return self.inspect_batch([lac])[0][0]
        except BatchDecodeError as e:
            raise RuntimeError(e.errors[0]) from None

    def check_batch(self, lacs, manifests, stream: int = 0) -> list:
        """Is each stream intact -- does every block decode to what its manifest says?  Per item (SalvageResult,
        [BlockFault]); a damaged or truncated stream (E_MISMATCH, "[check-error] block=N ..."), a manifest of another
        stream, a refused manifest or container raise BatchDecodeError once the others are done, with the results of the
        damaged ones in place (None for the others that failed)."""
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        n = len(bufs)
        spans = (Span * max(1, n))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        mspans, _keep = self._manifest_spans(manifests, n)
        res = (SalvageResult * max(1, n))()
        codes = []
        def call(rcs, ms):
            rc = lib().lacx_decoder_check_batch_device(self._h, spans, mspans, C.c_uint32(n), C.c_void_p(stream), rcs, res, ms)
            codes.extend(rcs[i] for i in range(n))
            return rc
        rc, errors = self._batch(n, call)
        results = [(self._copy_result(res[i]), self._faults(i)) if codes[i] == OK or (codes[i] == E_MISMATCH and res[i].blocks) else None
                   for i in range(n)]
        return self._raise_batch(rc, errors, results)

    # ---- recovery data: a parity sidecar that brings lost bytes back ----
    @staticmethod
    def _spans(blobs):
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in blobs]
        return (Span * max(1, len(bufs)))(*[Span(b.ctypes.data_as(C.POINTER(C.c_uint8)) if b.size else None, b.size) for b in bufs]), bufs

    def _bad_slices(self, i) -> list:
        ptr, count = C.POINTER(C.c_uint32)(), C.c_uint32()
        if lib().lacx_decoder_item_bad_slices(self._h, C.c_uint32(i), C.byref(ptr), C.byref(count)) != OK:
            return []
        return [int(ptr[k]) for k in range(count.value)]

    def recovery_build_batch(self, lacs, slice_bytes: int = 0, parity: int = 0, group_data: int = 0) -> list:
        """The recovery sidecar ("LACR") of each .lac file, all made as one device job; 0 = the default (4096, 8, 128).
        ValueError for parameters out of range; a file that stream_parse refuses raises BatchDecodeError once the others
        are done (results[i] is None there)."""
        spans, _keep = self._spans(lacs)
        n = len(lacs)
        if not (0 <= slice_bytes < 1 << 32 and 0 <= parity < 1 << 16 and 0 <= group_data < 1 << 16):
            raise ValueError("[recovery-error] parameters out of range")
        prm = RecoveryParams(slice_bytes, parity, group_data)
        outs = (Span * max(1, n))()
        codes = []

        def call(rcs, ms):
            rc = lib().lacx_recovery_build_batch_view(self._h, spans, C.c_uint32(n), C.byref(prm), outs, rcs, ms)
            codes.extend(rcs[i] for i in range(n))
            return rc
        rc, errors = self._batch(n, call)
        if rc == E_INVALID and all(c == OK for c in codes):  # the call's own arguments
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        return self._raise_batch(rc, errors, [None if (i in errors or not outs[i].data) else C.string_at(outs[i].data, outs[i].size) for i in range(n)])

    def recovery(self, lac, slice_bytes: int = 0, parity: int = 0, group_data: int = 0) -> bytes:
        """recovery_build_batch of one file; RuntimeError with the parser's message where the container is refused."""
        try:
            return self.recovery_build_batch([lac], slice_bytes, parity, group_data)[0]
        except BatchDecodeError as e:
            raise RuntimeError(e.errors[0]) from None

    def recovery_scan_batch(self, files, sidecars) -> list:
        """Where is each file damaged?  Per item (RepairResult, [damaged slices]); a damaged or truncated file (E_MISMATCH,
        "[recovery-error] slice=N bad_slices=M repairable|unrepairable") and a refused sidecar raise BatchDecodeError once
        the others are done, with the results of the damaged ones in place (None for a refused sidecar)."""
        if len(files) != len(sidecars):
            raise ValueError("one sidecar per file")
        n = len(files)
        fspans, _k1 = self._spans(files)
        sspans, _k2 = self._spans(sidecars)
        res = (RepairResult * max(1, n))()
        codes = []

        def call(rcs, ms):
            rc = lib().lacx_recovery_scan_batch(self._h, fspans, sspans, C.c_uint32(n), rcs, res, ms)
            codes.extend(rcs[i] for i in range(n))
            return rc
        rc, errors = self._batch(n, call)
        results = [(_copy_struct(res[i]), self._bad_slices(i)) if codes[i] in (OK, E_MISMATCH) else None for i in range(n)]
        return self._raise_batch(rc, errors, results)

    def repair_batch(self, files, sidecars, best_effort: bool = False) -> list:
        """Each file's original bytes, rebuilt from its recovery sidecar where it is damaged or cut short, all as one
        device job.  Per item (bytes or None, RepairResult, [damaged slices]).  An item with a group beyond its parity
        (E_MISMATCH, "[recovery-error] group G: B damaged slices, P parity slices usable"; bytes only with best_effort:
        every repairable group repaired, the rest as found), one whose repaired bytes miss the checksum and a refused
        sidecar (results[i] is None) raise BatchDecodeError once the others are done."""
        if len(files) != len(sidecars):
            raise ValueError("one sidecar per file")
        n = len(files)
        fspans, _k1 = self._spans(files)
        sspans, _k2 = self._spans(sidecars)
        res = (RepairResult * max(1, n))()
        outs = (Span * max(1, n))()
        codes = []

        def call(rcs, ms):
            rc = lib().lacx_recovery_repair_batch_view(self._h, fspans, sspans, C.c_uint32(n), C.c_uint32(REPAIR_BEST_EFFORT if best_effort else 0),
                                                       outs, rcs, res, ms)
            codes.extend(rcs[i] for i in range(n))
            return rc
        rc, errors = self._batch(n, call)
        results = [(C.string_at(outs[i].data, outs[i].size) if outs[i].data else None, _copy_struct(res[i]), self._bad_slices(i))
                   if codes[i] in (OK, E_MISMATCH) else None for i in range(n)]
        return self._raise_batch(rc, errors, results)

    def repair(self, file, sidecar, best_effort: bool = False):
        """repair_batch of one file: (bytes, RepairResult, [damaged slices]); RuntimeError with the item's message where it
        is not fully repaired (the partial answer in the exception's `result`) or the sidecar is refused."""
        try:
            return self.repair_batch([file], [sidecar], best_effort)[0]
        except BatchDecodeError as e:
            err = RuntimeError(e.errors[0])
            err.result = e.results[0]
            raise err from None

    def transcode_batch(self, encoder: "Encoder", outputs, verify: bool = False) -> list:
        """.lac in, .lac out, many outputs as one device job (lacx_transcode_batch): every output is a list of frame ranges
        of source streams, cut and joined, optionally re-channelled and re-quantised losslessly, and re-encoded by
        `encoder` (its zero-run and partitioning switches; its format is not used: rate, depth and channels come from the
        sources).  outputs[i]: a dict(segments=..., bit_depth=0, channels="keep", stereo_mode=2) or a tuple in that order;
        segments: a list of .lac bytes (the whole stream) or (lac, start, frames) with frames None = to the stream's end;
        bit_depth 0 keeps the sources', 16 / 24 change it where that loses nothing; channels: a CHANNEL_OPS name or a CH_*
        code.  verify: every new stream is decoded again on the device and compared with what it was encoded from.
        Returns [(bytes, EditResult)]; failed outputs raise BatchDecodeError once the others are done (errors[i] the
        output's message, results[i] None)."""
        if self._h is None:
            raise RuntimeError("decoder is closed")
        keep, segs, outs = [], [], []
        for o in outputs:
            if isinstance(o, dict):
                o = (o["segments"], o.get("bit_depth", 0), o.get("channels", "keep"), o.get("stereo_mode", 2))
            segments, depth, op, mode = (tuple(o) + (0, "keep", 2)[len(o) - 1:])[:4]
            first = len(segs)
            for sg in segments:
                lac, start, frames = (sg, 0, None) if isinstance(sg, (bytes, bytearray, memoryview, np.ndarray)) else sg
                b = np.frombuffer(lac, dtype=np.uint8)
                keep.append(b)
                segs.append(EditSegment(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size, int(start), TO_END if frames is None else int(frames)))
            outs.append(EditOutput(first, len(segs) - first, int(depth or 0), CHANNEL_OPS[op] if isinstance(op, str) else int(op), int(mode)))
        n = len(outs)
        seg_arr = (EditSegment * max(1, len(segs)))(*segs)
        out_arr = (EditOutput * max(1, n))(*outs)
        spans = (Span * max(1, n))()
        res = (EditResult * max(1, n))()
        rc, errors = self._batch(n, lambda rcs, ms: lib().lacx_transcode_batch(
            self._h, encoder._handle(), seg_arr, C.c_uint32(len(segs)), out_arr, C.c_uint32(n),
            C.c_uint32(TRANSCODE_VERIFY if verify else 0), spans, rcs, res, ms))
        results = []
        for i in range(n):
            if spans[i].data:
                data = C.string_at(spans[i].data, spans[i].size)
                lib().lacx_free(spans[i].data)
                results.append(None if i in errors else (data, _copy_struct(res[i])))
            else:
                results.append(None)
        if rc == E_INVALID and not errors:  # the whole call was refused
            raise ValueError(lib().lacx_decode_last_error().decode(errors="replace"))
        return self._raise_batch(rc, errors, results)

    def cut(self, encoder: "Encoder", lac, start: int, frames=None, verify: bool = False) -> bytes:
        """Frames [start, start + frames) of a .lac (frames None: to its end) as a .lac of their own."""
        return self.transcode_batch(encoder, [([(lac, start, frames)],)], verify)[0][0]

    def join(self, encoder: "Encoder", lacs, verify: bool = False) -> bytes:
        """Streams of one format, one behind the other, as one .lac."""
        return self.transcode_batch(encoder, [(list(lacs),)], verify)[0][0]

    def recompress(self, encoder: "Encoder", lac, bit_depth: int = 0, channels="keep", stereo_mode: int = 2, verify: bool = False) -> bytes:
        """A .lac coded again by `encoder` (a version-2 stream comes out as version 3), optionally re-channelled or
        re-quantised where that loses nothing."""
        return self.transcode_batch(encoder, [([lac], bit_depth, channels, stereo_mode)], verify)[0][0]

    def verify_wav(self, lac, wav) -> VerifyResult:
        """A .lac against the WAV file image it was made from (both in host memory): the image's data chunk goes to the
        device as it is and is compared there with the decoded stream.  Returns the VerifyResult -- a mismatch is an
        answer, not an exception: `identical` is False and `message` holds "[verify-error] ..." (also for a difference
        in format, where the counts stay zero and `format_differs` is set); kernel milliseconds in `last_ms`.  RuntimeError where the stream
        does not decode, ValueError for an image that is no PCM WAV."""
        if self._h is None:
            raise RuntimeError("decoder is closed")
        lbuf = np.frombuffer(lac, dtype=np.uint8)
        wbuf = np.frombuffer(wav, dtype=np.uint8)
        res = VerifyResult()
        ms = C.c_float()
        u8 = C.POINTER(C.c_uint8)
        rc = lib().lacx_decoder_verify_wav(self._h, lbuf.ctypes.data_as(u8), C.c_uint64(lbuf.size), wbuf.ctypes.data_as(u8),
                                           C.c_uint64(wbuf.size), C.byref(res), C.byref(ms))
        self.last_ms = float(ms.value)
        res.message = "" if rc == OK else lib().lacx_decode_last_error().decode(errors="replace")
        res.identical = rc == OK
        res.format_differs = rc == E_MISMATCH and res.mismatches == 0
        if rc in (OK, E_MISMATCH):
            return res
        if rc == E_INVALID and res.message.startswith("[verify-error]"):
            raise ValueError(res.message)
        raise RuntimeError(res.message)


def decode_wav(lac, device: int = -1) -> bytes:
    """Decoder(device).decode_wav(lac) for one stream: the WAV file image of a .lac, made on the device."""
    dec = Decoder(device)
    try:
        return dec.decode_wav(lac)
    finally:
        dec.close()


def assemble(sample_rate: int, bit_depth: int, stereo_mode: int, channels: int, shards) -> bytes:
    """Header + block table + payload concat of (payload, table) shards given in stream order
    (ref src/codec/lac/encoder.cpp:243-250, 445-465)."""
    cfg = Config(sample_rate, bit_depth, stereo_mode, 1, 1, -1, 0, 0)
    n = len(shards)
    pays = (C.c_char_p * n)(*[s[0] for s in shards])
    sizes = (C.c_uint64 * n)(*[len(s[0]) for s in shards])
    tabs_np = [np.ascontiguousarray(s[1], dtype=np.uint32) for s in shards]
    tabs = (C.POINTER(C.c_uint32) * n)(*[t.ctypes.data_as(C.POINTER(C.c_uint32)) for t in tabs_np])
    nbs = (C.c_uint32 * n)(*[t.shape[0] for t in tabs_np])
    out = C.POINTER(C.c_uint8)()
    size = C.c_uint64()
    rc = lib().lacx_assemble(C.byref(cfg), channels, n, C.cast(pays, C.POINTER(C.POINTER(C.c_uint8))), sizes, tabs,
                             nbs, C.byref(out), C.byref(size))
    if rc != OK:
        raise RuntimeError("lacx_assemble failed")
    return _take(out, size)


class BlockEncoder:
    """Mirror of Block::Encoder (ref src/codec/block/encoder.hpp:9-30)."""

    def __init__(self, order: int = 12, debug_lpc: bool = False, debug_zr: bool = False, device: int = -1):
        self._enc = Encoder(order, 0, 48000, 24, device=device)

    def set_zero_run_enabled(self, enabled: bool):
        self._enc.set_zero_run_enabled(enabled)

    def set_partitioning_enabled(self, enabled: bool):
        self._enc.set_partitioning_enabled(enabled)

    def set_debug_block_index(self, index: int):
        pass

    def set_debug_partitions(self, enabled: bool):
        pass

    def encode(self, pcm) -> bytes:
        P, pp = _i32(pcm)
        out = C.POINTER(C.c_uint8)()
        size = C.c_uint64()
        h = self._enc._handle()
        rc = lib().lacx_block_encode(h, pp, C.c_uint32(P.size), C.byref(out), C.byref(size))
        if rc != OK:
            _raise(h, rc)
        return _take(out, size)

    def plan(self, pcm) -> ChannelPlan:
        P, pp = _i32(pcm)
        plan = ChannelPlan()
        h = self._enc._handle()
        rc = lib().lacx_block_plan_only(h, pp, C.c_uint32(P.size), C.byref(plan))
        if rc != OK:
            _raise(h, rc)
        return plan

    def debug_lpc(self, pcm):
        P, pp = _i32(pcm)
        ac = np.zeros(13, dtype=np.int64)
        coef = np.zeros((5, 13), dtype=np.int16)
        used = np.zeros(5, dtype=np.uint8)
        h = self._enc._handle()
        rc = lib().lacx_debug_lpc(h, pp, C.c_uint32(P.size), ac.ctypes.data_as(C.POINTER(C.c_int64)),
                                  coef.ctypes.data_as(C.POINTER(C.c_int16)),
                                  used.ctypes.data_as(C.POINTER(C.c_uint8)))
        if rc != OK:
            _raise(h, rc)
        return ac, coef, used


class BatchItem(C.Structure):
    _fields_ = [("pcm", Pcm), ("frames", C.c_uint64), ("sample_rate", C.c_uint32), ("bit_depth", C.c_uint8),
                ("stereo_mode", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class BatchOut(C.Structure):
    _fields_ = [("payload", C.POINTER(C.c_uint8)), ("payload_size", C.c_uint64), ("table", C.POINTER(C.c_uint32)),
                ("nblocks", C.c_uint32), ("reserved", C.c_uint32)]


class BatchEncoder:
    """Many streams as ONE device job (lacx_encode_batch_device): every stream keeps its own rate, depth, channels and
    stereo mode.  formats: [(sample_rate, bit_depth, stereo_mode), ...] in the order the streams are passed later."""

    def __init__(self, formats, device: int = -1, zero_run: bool = True, partitioning: bool = True):
        self.formats = [tuple(f) for f in formats]
        self._enc = Encoder(12, 2, 48000, 16, device=device)
        self._enc.set_zero_run_enabled(zero_run)
        self._enc.set_partitioning_enabled(partitioning)

    def timing(self) -> Timing:
        return self._enc.timing()

    def encode_device(self, streams, stream: int = 0):
        """streams: [(data_ptr, layout, channels, frames[, data1_ptr]) or a device tensor (pcm_of), ...] device-resident PCM; returns a list of
        (PayloadView, table uint32[nblocks, 2]) views into the encoder's pinned result buffer."""
        n = len(streams)
        if n != len(self.formats):
            raise ValueError("one stream per format")
        items = (BatchItem * n)()
        for it, st, (sr, bd, sm) in zip(items, streams, self.formats):
            if isinstance(st, (tuple, list)):
                ptr, layout, ch, frames = st[:4]
                it.pcm = Pcm(ptr, st[4] if len(st) > 4 else None, layout, ch)
            else:  # a tensor, described by itself at the stream's bit depth (see pcm_of)
                it.pcm, frames = pcm_of(st, bd)
            it.frames = frames
            it.sample_rate = sr
            it.bit_depth = bd
            it.stereo_mode = sm
        outs = (BatchOut * n)()
        h = self._enc._handle()
        rc = lib().lacx_encode_batch_device(h, items, C.c_uint32(n), C.c_void_p(stream), outs)
        if rc != OK:
            _raise(h, rc)
        return [(PayloadView(o.payload, o.payload_size), TableView(o.table, o.nblocks)) for o in outs]


class TableView:
    """Borrowed view of a block table (frames, bytes per block) in encoder-owned pinned memory; converted to a numpy array
    only when asked (a batch of many streams returns one per stream on every call)."""

    def __init__(self, ptr, nblocks):
        self._ptr = ptr
        self.shape = (int(nblocks), 2)

    def array(self) -> np.ndarray:
        return np.ctypeslib.as_array(self._ptr, shape=self.shape)

    def copy(self) -> np.ndarray:
        return self.array().copy()

    def __array__(self, dtype=None, copy=None):
        a = self.array()
        return a.astype(dtype) if dtype is not None and a.dtype != dtype else a
