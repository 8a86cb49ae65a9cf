"""BGZF input on the host (csrc/sampost.cpp): mi355x_bgzf_scan, mi355x_bgzf_find_block and mi355x_bgzf_inflate on the
families and the malformed files of tests/bgzf_in_cases.py.  CPU only; the device path's entry points are looked at, not called
(tests/test_gpu_bgzf_inflate.py calls them)."""
import ctypes as C
import os
import re
import struct

import pytest

import bgzf_in_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(built):
    from mpibwa_amd import api
    return api.load_library()


def inflate(fn, data, cap=None):
    """(return value, text written)"""
    cap = sum(struct.unpack_from("<I", b, len(b) - 4)[0] for _, b in _whole_blocks(data)) + 64 if cap is None else cap
    out = C.create_string_buffer(max(cap, 1))
    n = fn(data, len(data), out, cap)
    return n, out.raw[:max(n, 0)]


def _whole_blocks(data):
    """the blocks that the framing gives, as far as it goes"""
    out, at = [], 0
    while at + 18 <= len(data) and data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00":
        n = struct.unpack_from("<H", data, at + 16)[0] + 1
        if at + n > len(data):
            break
        out.append((at, data[at:at + n]))
        at += n
    return out


def scan(lib, data, cap=None):
    cap = len(data) // 26 + 1 if cap is None else cap
    blk, txt = (C.c_int64 * (cap + 1))(), (C.c_int64 * (cap + 1))()
    n = lib.mi355x_bgzf_scan(data, len(data), cap, blk, txt)
    return n, list(blk[:max(n, 0) + 1]), list(txt[:max(n, 0) + 1])


def test_the_library_the_binding_and_the_header_declare_the_entry_points(lib):
    head = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mpibwa_amd.h")).read())
    for decl in ("int64_t mi355x_bgzf_find_block(const uint8_t *buf, int64_t len, int at_eof);",
                 "int64_t mi355x_bgzf_scan(const uint8_t *buf, int64_t len, int64_t cap, int64_t *blk_off, int64_t *text_off);",
                 "int64_t mi355x_bgzf_inflate(const uint8_t *in, size_t len, char *out, size_t cap);",
                 "int64_t mi355x_bgzf_inflate_dev(const uint8_t *in, size_t len, char *out, size_t cap);",
                 "void mi355x_bgzf_inflate_dev_counts(uint64_t out[4]);"):
        assert decl in head
    assert lib.mi355x_bgzf_inflate_dev.restype is C.c_int64
    c = (C.c_uint64 * 4)()
    lib.mi355x_bgzf_inflate_dev_counts(c)   # host code: nothing has to be on a device for it
    assert c[0] >= c[1]


def test_the_level_families_have_dynamic_codes_with_run_symbols():
    for level in (1, 6, 9):
        for _, blk in cases.split(cases.families()["level%d" % level][0]):
            btype, used = cases.dynamic_header(blk[18:-8])
            assert btype == 2 and {16, 17, 18} <= used


def test_scan_gives_the_block_table_of_the_families_one_after_the_other(lib):
    F = cases.families()
    data = b"".join(d for d, _ in F.values())
    n, blk, txt = scan(lib, data)
    parts = cases.split(data)
    assert n == len(parts) and blk == [o for o, _ in parts] + [len(data)]
    sizes = [struct.unpack_from("<I", b, len(b) - 4)[0] for _, b in parts]
    assert txt == [sum(sizes[:k]) for k in range(n + 1)] and txt[n] == sum(len(t) for _, t in F.values())
    assert sizes.count(0) >= 5   # (blocks of ISIZE 0 are blocks like any other, the EOF block in the middle included)
    # a cap below the number of blocks stops the walk; a block that the buffer cuts off ends it without an error
    assert scan(lib, data, cap=3)[0] == 3
    n2, blk2, _ = scan(lib, data[:blk[5] + 40])
    assert n2 == 5 and blk2[5] == blk[5]
    # a header that is not one
    assert scan(lib, data[:blk[2]] + b"\x55" * 30 + data[blk[2]:])[0] == -blk[2] - 1


def test_find_block_from_every_offset_finds_the_next_true_start(lib):
    fq = cases.fastq_text(600, seed=9)
    inner = cases.block(fq[:200])
    # a stored block that holds a header-looking sequence: a whole BGZF block, whose BSIZE hop leads to bytes that are no header
    planted = cases.block(b"xx" + inner + b"yy" * 40, level=0)
    assert inner in planted
    data = b"".join([cases.block(fq[:300]), planted, cases.block(fq[300:]), cases.EOF_BLOCK, cases.block(fq[:100]), cases.EOF_BLOCK])
    starts = [o for o, _ in cases.split(data)]
    false_start = data.index(inner)
    assert false_start not in starts
    for o in range(len(data)):
        want = min((s for s in starts if s >= o), default=None)
        got = lib.mi355x_bgzf_find_block(data[o:], len(data) - o, 1)
        assert got == (-1 if want is None else want - o), o
    # without the end of the file in sight, a candidate whose chain leaves the buffer cannot be decided
    assert lib.mi355x_bgzf_find_block(data, starts[2] + 5, 0) == -2
    assert lib.mi355x_bgzf_find_block(data, len(data), 0) == 0
    assert lib.mi355x_bgzf_find_block(b"\x00" * 100, 100, 0) == -1


def test_the_host_inflate_gives_zlibs_text_on_every_family(lib):
    for name, (data, text) in cases.families().items():
        n, got = inflate(lib.mi355x_bgzf_inflate, data)
        assert n == len(text) and got == text, name
    data = b"".join(d for d, _ in cases.families().values())
    text = b"".join(t for _, t in cases.families().values())
    assert inflate(lib.mi355x_bgzf_inflate, data) == (len(text), text)
    # a cap one byte short gives 0 and writes nothing
    out = C.create_string_buffer(b"\xaa" * len(text), len(text))
    assert lib.mi355x_bgzf_inflate(data, len(data), out, len(text) - 1) == 0 and out.raw == b"\xaa" * len(text)


def test_the_host_inflate_reports_the_first_failing_block_of_every_malformed_file(lib):
    for name, (data, off) in cases.malformed().items():
        assert inflate(lib.mi355x_bgzf_inflate, data)[0] == -off - 1, name
    # two bad blocks: the first one is reported
    a, _ = cases.malformed()["crc_one_bit"]
    b, off_b = cases.malformed()["btype_3"]
    assert inflate(lib.mi355x_bgzf_inflate, b + a)[0] == -off_b - 1


def test_the_round_trip_through_the_librarys_own_compressor(lib):
    text = cases.fastq_text(200000, seed=11)
    for level in (1, 6, 0):
        cap = lib.mi355x_bgzf_bound(len(text))
        out = C.create_string_buffer(cap)
        n = lib.mi355x_bgzf_compress(text, len(text), level, out, cap)
        assert n > 0
        assert inflate(lib.mi355x_bgzf_inflate, out.raw[:n]) == (len(text), text)
