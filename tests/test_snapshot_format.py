"""The snapshot format (include/lcx_state.h, csrc/lcx_snapshot_format.hpp) where it needs no device: the checksum against its
restatement in numpy, lcx_snapshot_describe's refusals, and the format's writer and validating reader in a program of their own under
the host sanitizers."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _harness as h  # noqa: F401  (as in every test module)
from libcloudphxx_amd import _lib, lgrngn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 2 ** 16 + 3]


def checksum_numpy(data):
    """include/lcx_state.h: the sum modulo 2^64 over the 8-byte little-endian words w_i (the tail padded with zeros) of
    mix(w_i + (i + 1) * GOLDEN), mix = splitmix64's finaliser.  numpy's uint64 array arithmetic wraps."""
    b = np.frombuffer(bytes(data), dtype=np.uint8)
    pad = np.zeros((-len(b)) % 8, dtype=np.uint8)
    w = np.concatenate([b, pad]).view("<u8").astype(np.uint64)
    with np.errstate(over="ignore"):
        z = w + (np.arange(len(w), dtype=np.uint64) + np.uint64(1)) * GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return int(z.sum(dtype=np.uint64))


def seeded(n):
    return np.random.default_rng(20261019 + n).integers(0, 256, size=n, dtype=np.uint8)


def checksum_host(lib, a):
    out = C.c_ulonglong()
    a = np.ascontiguousarray(a, dtype=np.uint8)
    assert lib.lcx_snapshot_checksum_host(C.c_void_p(a.ctypes.data if a.size else None), C.c_size_t(a.size), C.byref(out)) == 0
    return out.value


def test_the_library_loads_without_a_device_and_has_the_entries():
    lib = _lib.load()
    for name in ("size", "save", "load", "describe", "checksum_host", "checksum_probe"):
        assert hasattr(lib, "lcx_snapshot_" + name), name


@pytest.mark.parametrize("n", LENGTHS)
def test_host_checksum_is_the_numpy_restatement(n):
    a = seeded(n)
    assert checksum_host(_lib.load(), a) == checksum_numpy(a)
    if n == 0:
        assert checksum_numpy(a) == 0


def test_two_words_swapped_change_the_checksum():
    lib = _lib.load()
    a = seeded(64)
    b = a.copy()
    b[8:16], b[40:48] = a[40:48], a[8:16]
    assert not np.array_equal(a, b)
    assert checksum_host(lib, a) != checksum_host(lib, b)
    assert checksum_host(lib, b) == checksum_numpy(b)
    # a tail byte counts, and so does the length (a trailing zero BYTE inside the same word does not: the word is padded with zeros)
    c = seeded(65)
    d = c.copy()
    d[64] ^= 1
    assert checksum_host(lib, c) != checksum_host(lib, d)


# ---- a synthetic blob, laid out by hand from the documented structs: header 256 B, named values 40 B, table entries 64 B ----
def name32(s):
    return s.encode().ljust(32, b"\0")


def synthetic_blob(version=1, magic=b"LCXSNAP1", section_count=10, section_offset=None):
    opts = [("nx", 4), ("strict_fp", 1)]
    scalars = [("n_part", 9), ("n_storage", 10), ("n_cell", 8), ("rng_call", 3)]
    head = 256 + 40 * (len(opts) + len(scalars)) + 64
    data_off = (head + 63) // 64 * 64
    payload = seeded(10 * 8).tobytes()
    total = data_off + (len(payload) + 63) // 64 * 64
    off = data_off if section_offset is None else section_offset
    table = name32("n") + struct.pack("<IIQQQ", 0, 8, section_count, off, checksum_numpy(payload))
    body = b"".join(name32(k) + struct.pack("<Q", v) for k, v in opts + scalars) + table

    def header(cks):
        return (magic + struct.pack("<IIQIIII", version, 256, total, 8, len(opts), len(scalars), 1) +
                struct.pack("<QQQQQQ", 256, 256 + 40 * len(opts), 256 + 40 * (len(opts) + len(scalars)), data_off, 32 << 20, cks) +
                b"synthetic".ljust(64, b"\0") + bytes(104))
    pad = bytes(data_off - head)
    cks = checksum_numpy(header(0) + body + pad)
    blob = header(cks) + body + pad + payload
    return np.frombuffer(blob.ljust(total, b"\0"), dtype=np.uint8).copy()


def test_describe_accepts_a_blob_laid_out_from_the_documented_structs():
    text = lgrngn.snapshot_describe(synthetic_blob())
    assert "format 1" in text and "synthetic" in text and "real kind 8" in text
    assert "n_storage = 10" in text and "n_cell = 8" in text and "rng_call = 3" in text
    assert "section n: uint64 x 10" in text


@pytest.mark.parametrize("case,needle", [
    ("empty", "truncated"), ("magic", "wrong magic"), ("future", "version 2 is unknown"), ("overrun_count", "section 'n' overruns the blob"),
    ("overrun_offset", "section 'n' overruns the blob"), ("cut", "truncated"), ("head_bit", "header checksum does not match")])
def test_describe_refuses(case, needle):
    blob = {"empty": lambda: np.zeros(0, dtype=np.uint8), "magic": lambda: synthetic_blob(magic=b"LCXSNAPX"), "future": lambda: synthetic_blob(version=2),
            "overrun_count": lambda: synthetic_blob(section_count=1000), "overrun_offset": lambda: synthetic_blob(section_offset=1 << 40),
            "cut": lambda: synthetic_blob()[:-1], "head_bit": lambda: synthetic_blob()}[case]()
    if case == "head_bit":
        blob[300] ^= 4                      # (inside an option's name)
    with pytest.raises(RuntimeError) as e:
        lgrngn.snapshot_describe(blob)
    assert str(e.value).startswith("libcloudph++: ") and needle in str(e.value), str(e.value)


def test_format_header_alone_under_the_host_sanitizers(tmp_path):
    """tools/snapshot_format_check.cpp: the format's own writer and reader in a program of their own -- a synthetic blob, every
    truncation of it and every single head byte altered -- built with -fsanitize=address,undefined.  Host code, run as a child process."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "snapshot_format_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "snapshot_format_check.cpp")], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
