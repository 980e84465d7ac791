"""The reference's answers to the calls the oracle-vs-reference tests make, pinned in tests/golden/ref_answers.json.

Those tests compare the oracle with the unmodified reference build (oracle/_ref, see refshim.py), which exists only where
the reference sources were present when the checkers were built.  reference() hands the tests an object with refshim's
interface in every case:

  * oracle/_ref present: the live reference; every answer is also checked against the pinned one, so a stale
    fixture fails loudly;
  * oracle/_ref absent: the pinned answers.  Byte strings and sample arrays come back as Pinned values (length/shape +
    sha256) that compare equal to exactly the bytes / samples the reference returned; small results come back as
    they are;
  * LACX_REF_RECORD=1 (with oracle/_ref present): the live reference, and the answers are written to the fixture when
    the process ends:  LACX_REF_RECORD=1 python -m pytest tests/test_oracle_vs_ref.py tests/test_wav_ingest.py \
                                                          tests/test_lacgrammar_host.py

A decode the reference refuses is an answer too: it is pinned with its message and replayed as the same RuntimeError.

Calls are keyed by the function name and a digest of their arguments (arrays by value, a WAV path by file content).
"""
from __future__ import annotations

import atexit
import hashlib
import inspect
import json
import os

import numpy as np

import refshim

ANSWERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_answers.json")


def _array_digest(a) -> str:
    a = np.asarray(a)
    h = hashlib.sha256(f"{a.shape}".encode())
    h.update(np.ascontiguousarray(a, dtype=np.int64).tobytes())
    return h.hexdigest()


class Pinned:
    """A reference result known by its digest: equal to bytes / an integer array with exactly that content."""

    def __init__(self, kind: str, size: int, sha: str):
        self.kind, self.size, self.sha = kind, size, sha

    def matches(self, other) -> bool:
        if isinstance(other, Pinned):
            return (self.kind, self.size, self.sha) == (other.kind, other.size, other.sha)
        if self.kind == "bytes":
            return isinstance(other, (bytes, bytearray)) and len(other) == self.size and \
                hashlib.sha256(other).hexdigest() == self.sha
        return np.asarray(other).size == self.size and _array_digest(other) == self.sha

    def __eq__(self, other):
        return self.matches(other)

    def __ne__(self, other):
        return not self.matches(other)

    __hash__ = None

    def __repr__(self):
        return f"<reference {self.kind}: {self.size} items, sha256 {self.sha[:16]}>"


def same(a, b) -> bool:
    """np.array_equal that also accepts a Pinned array on either side."""
    if isinstance(b, Pinned):
        return b.matches(a)
    if isinstance(a, Pinned):
        return a.matches(b)
    return np.array_equal(a, b)


def _enc(v):
    """JSON form of a result."""
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, Pinned):
        return {"pinned": v.kind, "size": v.size, "sha256": v.sha}
    if isinstance(v, (bytes, bytearray)):
        return {"pinned": "bytes", "size": len(v), "sha256": hashlib.sha256(v).hexdigest()}
    if isinstance(v, np.ndarray):
        return {"pinned": "array", "size": int(v.size), "sha256": _array_digest(v)}
    if isinstance(v, (tuple, list)):
        return {"tuple": [_enc(x) for x in v]}
    if isinstance(v, dict):
        return {"dict": {k: _enc(x) for k, x in v.items()}}
    raise TypeError(f"cannot pin a {type(v).__name__}")


def _dec(j):
    if isinstance(j, dict):
        if "pinned" in j:
            return Pinned(j["pinned"], j["size"], j["sha256"])
        if "tuple" in j:
            return tuple(_dec(x) for x in j["tuple"])
        if "dict" in j:
            return {k: _dec(x) for k, x in j["dict"].items()}
    return j


def _arg_digest(v) -> str:
    if isinstance(v, np.ndarray):
        return "a" + _array_digest(v)
    if isinstance(v, (bytes, bytearray)):
        return "b" + hashlib.sha256(v).hexdigest()
    if isinstance(v, (np.integer,)):
        v = int(v)
    return "v" + repr(v)


def _key(name, args, kwargs) -> str:
    fn = getattr(refshim, name)
    bound = inspect.signature(fn).bind(*args, **kwargs)
    bound.apply_defaults()
    parts = [name]
    for k, v in bound.arguments.items():
        if name == "read_wav" and k == "path":
            with open(v, "rb") as f:
                v = f.read()
        parts.append(f"{k}={_arg_digest(v)}")
    return hashlib.sha256("|".join(parts).encode()).hexdigest()


# the refshim calls the tests make; lpc_analyze's coefficients are small enough to keep as they are
_CALLS = ("encode", "decode", "block_encode", "lpc_analyze", "adapt_k_sequence", "read_wav")


class _Reference:
    def __init__(self, mode: str):
        self.mode = mode  # "live" (checked against the fixture), "record" or "replay"
        self.answers = {}
        if os.path.exists(ANSWERS):
            with open(ANSWERS) as f:
                self.answers = json.load(f)
        if mode == "record":
            self.recorded = {}
            atexit.register(self._write)

    def _write(self):
        merged = {}
        if os.path.exists(ANSWERS):
            with open(ANSWERS) as f:
                merged = json.load(f)
        merged.update(self.recorded)
        with open(ANSWERS, "w") as f:
            json.dump(dict(sorted(merged.items())), f, indent=0, sort_keys=True)
            f.write("\n")

    def _call(self, name, args, kwargs):
        key = _key(name, args, kwargs)
        if self.mode == "replay":
            if key not in self.answers:
                raise KeyError(f"no pinned reference answer for this {name} call: re-record {ANSWERS} where oracle/_ref exists")
            return _pinned_result(name, _dec(self.answers[key]))
        refusal = None
        try:
            got = getattr(refshim, name)(*args, **kwargs)
        except RuntimeError as err:
            if name != "decode":
                raise
            got, refusal = Refused(str(err)), err
        if self.mode == "record":
            self.recorded[key] = _enc_result(name, got)
        elif key not in self.answers or self.answers[key] != _enc_result(name, got):
            raise AssertionError(f"{ANSWERS} does not hold the reference's answer to this {name} call: re-record it")
        if refusal is not None:
            raise refusal
        return got

    def __getattr__(self, name):
        if name not in _CALLS:
            raise AttributeError(name)
        return lambda *args, **kwargs: self._call(name, args, kwargs)


class Refused:
    """A decode the reference refused: pinned with its message, replayed as the RuntimeError the live call raises."""

    def __init__(self, message: str):
        self.message = message


def _enc_result(name, got):
    if isinstance(got, Refused):
        return {"refused": got.message}
    if name == "lpc_analyze":  # (orders used, int16 coefficients) kept by value
        return {"tuple": [int(got[0]), [int(x) for x in got[1]]]}
    return _enc(got)


def _pinned_result(name, v):
    if isinstance(v, dict) and "refused" in v:
        raise RuntimeError(v["refused"])
    if name == "lpc_analyze":
        used, co = v
        return used, np.asarray(co, dtype=np.int16)
    return v


_instance = None


def reference():
    """The reference for the oracle tests: live where oracle/_ref exists, the pinned answers elsewhere."""
    global _instance
    if _instance is None:
        if refshim.available():
            _instance = _Reference("record" if os.environ.get("LACX_REF_RECORD") == "1" else "live")
        else:
            _instance = _Reference("replay")
    return _instance
