"""The device BGZF path's interface, and the one cut rule that it shares with the host path (csrc/sampost.cpp: bgzf_cuts).  CPU only:
the entry points are looked at, not called (they need an MI355X: tests/test_gpu_bgzf.py).

The host path's bytes must not have moved when the cut loop moved into a function of its own: the outputs of mi355x_bgzf_compress for
the texts of tests/test_sampost.py::test_bgzf_blocks_hold_whole_records_and_decompress_to_the_text are hashed against values recorded
from the library of the commit before (zlib 1.2.11, the system's)."""
import ctypes as C
import hashlib
import os
import re
import struct
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(built):
    from mpibwa_amd import api
    return api.load_library()


def test_the_library_the_binding_and_the_header_declare_the_device_entry_points(lib):
    f = lib.mi355x_bgzf_compress_dev
    assert f.restype is C.c_size_t and list(f.argtypes) == [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
    g = lib.mi355x_bgzf_dev_counts
    assert g.restype is None and list(g.argtypes) == [C.POINTER(C.c_uint64)]
    head = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mpibwa_amd.h")).read())
    assert "size_t mi355x_bgzf_compress_dev(const char *text, size_t len, uint8_t *out, size_t cap);" in head
    assert "void mi355x_bgzf_dev_counts(uint64_t out[4]);" in head
    # counting is host code and starts at zero or above; nothing has to be on a device for it
    c = (C.c_uint64 * 4)()
    g(c)
    assert c[0] >= c[1] and c[2] >= 0 and c[3] >= 0


def _texts():
    """the five texts of the host test, built the same way from the same seed"""
    rng = np.random.default_rng(4)

    def record(n):
        return b"r%d\t99\tchr1\t%d\t60\t%dM\t=\t%d\t400\t" % (n, n * 7, 150, n * 7 + 250) + bytes(rng.choice(list(b"ACGT"), 150).tolist()) + b"\t" + \
            bytes((rng.integers(2, 42, 150) + 33).astype(np.uint8).tolist()) + b"\tNM:i:0\tMD:Z:150\tAS:i:150\tXS:i:0\n"
    text = b"".join(record(n) for n in range(4000))
    long_line = b"x\t4\t*\t0\t0\t*\t*\t0\t0\t" + b"A" * 200000 + b"\t" + b"I" * 200000 + b"\n"
    return [text, b"", record(1), text[:70000] + long_line + text[70000:140000], bytes(rng.integers(0, 256, 300000).astype(np.uint8).tolist())]


# sha256 (first 16 hex digits) of mi355x_bgzf_compress's output per level and text, from the parent commit's library
PARENT = {
    -1: ["9f40d80078472e97", "e3b0c44298fc1c14", "19839a2d13378fdc", "f1aba16402d19458", "0e9d7b15431840a6"],
    1: ["5785ae3377e4e83f", "e3b0c44298fc1c14", "79765f81f6347083", "26871b0d786f3a0e", "4d4ba1570a5b54d9"],
    9: ["9265cea2d31dd19c", "e3b0c44298fc1c14", "19839a2d13378fdc", "38eecc0057e01ad9", "0e9d7b15431840a6"],
    0: ["69a382f0bc4d2b0f", "e3b0c44298fc1c14", "d5f8ceb39291ff2a", "c08a42a86d3f4bd8", "faf033ff83c6a06b"],
}


def _payload_lengths(data):
    out, at = [], 0
    while at < len(data):
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append(struct.unpack_from("<I", data, at + bsize - 4)[0])
        at += bsize
    return out


def test_the_host_path_writes_the_bytes_it_wrote_before_the_cut_loop_moved(lib):
    texts = _texts()
    assert hashlib.sha256(texts[0]).hexdigest() == "1fdd28194a1a98daf668817d50c083f5c77ba0afb9724f99592c7a2c08fc5e63"   # (the generator itself)
    cuts = []
    for level, want in PARENT.items():
        got = []
        for t in texts:
            cap = lib.mi355x_bgzf_bound(len(t))
            out = C.create_string_buffer(max(cap, 1))
            n = lib.mi355x_bgzf_compress(t, len(t), level, out, cap)
            got.append(hashlib.sha256(out.raw[:n]).hexdigest()[:16])
            if level == 0:
                cuts.append(_payload_lengths(out.raw[:n]))
        assert got == want, level
    # the rule itself, stated again: at most 0xff00 bytes, cut back to the last newline where the window has one
    for t, lens in zip(texts, cuts):
        at, want = 0, []
        while at < len(t):
            n = min(0xff00, len(t) - at)
            if at + n < len(t):
                nl = t.rfind(b"\n", at, at + n)
                if nl >= 0:
                    n = nl - at + 1
            want.append(n)
            at += n
        assert lens == want
    assert zlib.ZLIB_RUNTIME_VERSION   # (the hashes above are this zlib's bytes at levels 1, 6 and 9; level 0 is stored blocks)
