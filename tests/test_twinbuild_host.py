"""tests/twinbuild.py, the one way the CPU twins are built: a target is rebuilt exactly when a file the compiler read for it
is newer or gone -- never a list of headers kept by hand -- and a twin that cannot be rebuilt fails instead of running
the binary it has."""
import ctypes as C
import glob
import os
import shutil
import time
from concurrent.futures import ThreadPoolExecutor

import pytest

import blockdigesttwin
import dectwin
import digesttwin
import importtwin
import recoverytwin
import salvagetwin
import twinbuild
import vertwin


def _later(path, seconds=10):
    t = time.time() + seconds
    os.utime(path, (t, t))


def test_rebuilds_when_a_header_moves_and_fails_when_it_is_gone(tmp_path):
    src, head = tmp_path / "two.cpp", tmp_path / "own.h"
    head.write_text("#define ANSWER 41\n")
    src.write_text('#include "own.h"\nextern "C" int answer() { return ANSWER; }\n')
    build = str(tmp_path / "_build")
    so = twinbuild.shared_lib("two", [str(src)], build=build)
    assert os.path.exists(so + ".d") and str(head) in open(so + ".d").read()
    assert C.CDLL(so).answer() == 41
    built = os.stat(so).st_mtime_ns
    assert twinbuild.shared_lib("two", [str(src)], build=build) == so and os.stat(so).st_mtime_ns == built, "the second call rebuilt"
    head.write_text("#define ANSWER 42\n")
    _later(head)
    twinbuild.shared_lib("two", [str(src)], build=build)
    assert os.stat(so).st_mtime_ns != built, "a newer header did not rebuild"
    os.remove(so + ".d")  # no record of what was read: stale
    built = os.stat(so).st_mtime_ns
    twinbuild.shared_lib("two", [str(src)], build=build)
    assert os.stat(so).st_mtime_ns != built and os.path.exists(so + ".d")
    head.unlink()
    with pytest.raises(AssertionError, match="own.h"):
        twinbuild.shared_lib("two", [str(src)], build=build)  # not the old binary


def test_the_sanitized_program_goes_by_the_same_rule(tmp_path):
    head, main, build = tmp_path / "own.h", tmp_path / "main.cpp", str(tmp_path / "_build")
    head.write_text("#define ANSWER 43\n")
    main.write_text('#include "own.h"\nint main() { return ANSWER - 43; }\n')
    exe, why = twinbuild.sanitized_exe("two_san", [str(main)], build=build)
    if exe is None:
        pytest.skip(why)
    built = os.stat(exe).st_mtime_ns
    assert twinbuild.sanitized_exe("two_san", [str(main)], build=build) == (exe, "") and os.stat(exe).st_mtime_ns == built
    _later(head)
    twinbuild.sanitized_exe("two_san", [str(main)], build=build)
    assert os.stat(exe).st_mtime_ns != built
    head.unlink()
    with pytest.raises(AssertionError, match="own.h"):
        twinbuild.sanitized_exe("two_san", [str(main)], build=build)


def test_an_edit_to_manifest_h_rebuilds_the_decode_family(tmp_path):
    """decode_plan.h includes manifest.h: the decode, salvage and block digest twins are built from it, plain and sanitized,
    and must be rebuilt when it moves; a twin is rebuilt exactly when its .d names the file.  The edit is to a scratch copy
    of the headers on an include path ahead of csrc -- never to the tree."""
    twins = {"sim_decode": dectwin.SRC, "sim_salvage": salvagetwin.SRC, "sim_blockdigest": blockdigesttwin.SRC, "sim_digest": digesttwin.SRC,
             "sim_verify": vertwin.SRC, "sim_import": importtwin.SRC, "sim_recovery": recoverytwin.SRC}
    heads = tmp_path / "csrc"
    heads.mkdir()
    for h in glob.glob(os.path.join(twinbuild.CSRC, "*.h")):
        shutil.copy(h, heads)
    copy, build = str(heads / "manifest.h"), str(tmp_path / "_build")

    def both(name):  # -> {target: its mtime}, the sanitized program only where the runtime exists
        so = twinbuild.shared_lib(name, [twins[name]], include=[str(heads)], build=build)
        exe, _ = twinbuild.sanitized_exe(name + "_san", [twins[name]], ["-DSIM_%s_MAIN" % name[4:].upper()], include=[str(heads)], build=build)
        return {t: os.stat(t).st_mtime_ns for t in (so, exe) if t}

    def everything():
        with ThreadPoolExecutor(len(twins)) as pool:
            return {t: m for got in pool.map(both, twins) for t, m in got.items()}

    first = everything()
    reads = {t: copy in open(t + ".d").read().replace("\\\n", " ").split() for t in first}
    for name in ("sim_decode", "sim_salvage", "sim_blockdigest"):
        assert reads[os.path.join(build, "lib%s.so" % name)], name + " is not built from manifest.h"
    assert everything() == first, "a second call rebuilt something"
    _later(copy)
    again = everything()
    for t in first:
        assert (again[t] != first[t]) == reads[t], t + (" was not rebuilt" if reads[t] else " was rebuilt without cause")
