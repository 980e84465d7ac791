#!/usr/bin/env python3
"""Pins `lacx_cli decode` (lacx_decoder_decode_wav) to the UNMODIFIED reference CLI's `lac_cli decode`.  Run in the
build container only, where the reference sources exist:

    make -C oracle ref && python tests/golden/make_decode_wav_golden.py [/path/to/reference]

The reference CLI (src/main.cpp + the library sources oracle/Makefile lists as REF_SRCS) is compiled with g++ into a
temporary directory outside the repository and thrown away afterwards; oracle/ is not touched.

Outputs (committed): tests/golden/decode_wav/*.lac  small reference-encoded streams (refshim.encode) that the older
                                                     fixtures lack: odd data size (pad byte), forced MS 24-bit, mono
                                                     16-bit with a short final block, three-block LR
                     tests/golden/decode_wav.json    per stream: its source (a fixture, or a lacstreams recipe: version-2
                                                     rewrite, block range, splice), the generator parameters of its PCM,
                                                     and the reference CLI's WAV: length, sha256, header, stdout line
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as ge  # noqa: E402
import lacstreams  # noqa: E402
import refshim  # noqa: E402

synth = ge.load_pkg().synth
OUT_DIR = os.path.join(HERE, "decode_wav")

NEW = [
    # name, frames, channels, bit_depth, rate, stereo_mode, kind, stereo, seed
    ("mono24_16641_pad", 16384 + 257, 1, 24, 48000, 0, "tone", "wide", 21),
    ("st24_ms_20481", 16384 + 4097, 2, 24, 96000, 1, "tone", "narrow", 22),
    ("mono16_16639", 16384 + 255, 1, 16, 44100, 0, "sparse", "wide", 23),
    ("st16_lr_3blk", 2 * 16384 + 1000, 2, 16, 48000, 0, "silence", "identical", 24),
]


def ref_sources(ref):
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    block = re.search(r"REF_SRCS\s*=((?:.*\\\n)*.*)", mk).group(1)
    return [os.path.join(ref, p.replace("$(REF)/", "")) for p in re.findall(r"\$\(REF\)/\S+", block)]


def build_ref_cli(ref, tmp):
    exe = os.path.join(tmp, "lac_cli")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-pthread", "-I" + os.path.join(ref, "src"),
                           "-I" + os.path.join(ref, "include"), os.path.join(ref, "src", "main.cpp")] + ref_sources(ref)
                          + ["-o", exe])
    return exe


def read_fixture(name):
    with open(os.path.join(HERE, name), "rb") as f:
        return f.read()


def pcm_segments(recipe, gens):
    """[(gen, first frame, end frame)] of the PCM a recipe's stream decodes to."""
    if "file" in recipe:
        g = gens[recipe["file"]]
        if "blocks" in recipe:
            a, b = lacstreams.frame_ranges(read_fixture(recipe["file"]), *recipe["blocks"])
        else:
            a, b = 0, g["frames"]
        return [{"gen": g, "start": a, "end": b}]
    if "v2" in recipe:
        return pcm_segments(recipe["v2"], gens)
    return [s for r in recipe["splice"] for s in pcm_segments(r, gens)]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    assert refshim.available(), "build oracle/_ref/liblac_ref.so first: make -C oracle ref"
    os.makedirs(OUT_DIR, exist_ok=True)
    gens = {}
    with open(os.path.join(HERE, "small", "index.json")) as f:
        for ent in json.load(f):
            gens["small/" + ent["name"] + ".lac"] = ent["gen"]
    for name, frames, ch, bd, sr, sm, kind, stereo, seed in NEW:
        left, right = synth.synth_pcm(frames, ch, bd, sr, seed=seed, kind=kind, stereo=stereo)
        lac = refshim.encode(left, right, sr, bd, sm, threads=8)
        with open(os.path.join(OUT_DIR, name + ".lac"), "wb") as f:
            f.write(lac)
        gens["decode_wav/" + name + ".lac"] = dict(frames=frames, channels=ch, bit_depth=bd, sample_rate=sr, seed=seed,
                                                   kind=kind, stereo=stereo)
    streams = [(k[len("small/"):-4], {"file": k}) for k in sorted(gens) if k.startswith("small/")]
    streams += [(n, {"file": "decode_wav/" + n + ".lac"}) for n, *_ in NEW]
    streams += [
        ("v2_mono24_16641_pad", {"v2": {"file": "decode_wav/mono24_16641_pad.lac"}}),
        ("v2_st16_lr_3blk", {"v2": {"file": "decode_wav/st16_lr_3blk.lac"}}),
        # a 257-frame block (odd, 24-bit mono: every unit of four frames after it is shifted by 3 bytes) inside the stream
        ("splice_mono24_257_first", {"splice": [{"file": "decode_wav/mono24_16641_pad.lac", "blocks": [1, 2]},
                                                {"file": "decode_wav/mono24_16641_pad.lac"}]}),
        # a 4097-frame non-final block between 16384-frame ones, forced mid/side
        ("splice_st24_ms_4097_mid", {"splice": [{"file": "decode_wav/st24_ms_20481.lac", "blocks": [0, 1]},
                                                {"file": "decode_wav/st24_ms_20481.lac", "blocks": [1, 2]},
                                                {"file": "decode_wav/st24_ms_20481.lac"}]}),
        ("splice_st16_ms_257_257", {"splice": [{"file": "small/n257_st16_ms.lac"}, {"file": "small/n257_st16_ms.lac"}]}),
        ("splice_st16_4097_16384_37", {"splice": [{"file": "small/n4097_st16.lac"}, {"file": "small/n16421_st16.lac"}]}),
        ("v2_splice_mono16_3blk", {"v2": {"splice": [{"file": "decode_wav/mono16_16639.lac", "blocks": [0, 1]},
                                                     {"file": "decode_wav/mono16_16639.lac"}]}}),
    ]
    entries = []
    with tempfile.TemporaryDirectory() as tmp:
        cli = build_ref_cli(ref, tmp)
        for name, src in streams:
            lac = lacstreams.from_recipe(src, read_fixture)
            lp, wp = os.path.join(tmp, "in.lac"), os.path.join(tmp, "out.wav")
            with open(lp, "wb") as f:
                f.write(lac)
            res = subprocess.run([cli, "decode", lp, wp], capture_output=True, text=True)
            if res.returncode != 0:
                raise SystemExit(f"{name}: reference CLI failed: {res.stderr.strip()}")
            with open(wp, "rb") as f:
                wav = f.read()
            os.remove(wp)
            entries.append({
                "name": name,
                "source": src,
                "lac_sha256": hashlib.sha256(lac).hexdigest(),
                "pcm": pcm_segments(src, gens),
                "wav_bytes": len(wav),
                "wav_sha256": hashlib.sha256(wav).hexdigest(),
                "header_hex": wav[:44].hex(),
                "stdout": res.stdout.replace(lp, "{in}").replace(wp, "{out}"),
            })
    with open(os.path.join(HERE, "decode_wav.json"), "w") as f:
        json.dump(entries, f, indent=1)
        f.write("\n")
    total = sum(os.path.getsize(os.path.join(OUT_DIR, n + ".lac")) for n, *_ in NEW)
    print(f"{len(entries)} streams pinned; new fixtures {total} bytes")


if __name__ == "__main__":
    main()
