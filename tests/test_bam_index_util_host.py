"""csrc/bam_index_util.h on the host, through tests/csrc/bam_index_host_check.cpp (a program of its own: nothing is loaded into Python):
every record's contig, beg, end, bin and mapped bit against tests/bam_index_model.py, its virtual offset under cuts the program chooses,
and a stream cut anywhere refused without a read past its end.  The program is built with the address and undefined-behaviour
sanitizers where the compiler has their runtimes (every stream is a heap block of its exact size)."""
import os
import struct
import subprocess

import pytest

import bam_index_cases as ic
import bam_index_model as mi
import bam_model as bm
import bam_sort_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "bam_index_host_check.cpp")
INC = os.path.join(ROOT, "mpibwa_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_index_host")
    exe = str(d / "bam_index_host_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", INC, SRC, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:
        subprocess.run(base, check=True)
    return exe, san.returncode == 0, d


def _fnv(h, t):
    for b in t:
        h = ((h ^ b) * 16777619) & 0xffffffff
    return h


def _run(program, streams, name):
    exe, _, d = program
    path = str(d / name)
    with open(path, "wb") as f:
        for s in streams:
            f.write(struct.pack("<I", len(s)) + s)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(streams)
    return [(int(c), int(n), int(n_long), int(h, 16)) for c, n, n_long, h in rows]


def _want(stream):
    _, _, at = bm.decode_header(stream)
    h, n, n_long = 2166136261, 0, 0
    for r in bm.split_records(stream, at):
        ref, beg, end, mapped = mi.interval(r)
        b = mi.reg2bin(beg, min(end, mi.LIMIT + 1)) if ref >= 0 else 0
        block = at // 1000
        v0 = (block + (block >= 1)) << 16 | at % 1000      # (the program's cuts: every 1000 bytes, block 1 empty)
        h = _fnv(h, struct.pack("<QqQQQQQ", at, ref, beg, end, b, int(mapped), v0))
        n_long += end > mi.LIMIT
        at += len(r)
        n += 1
    return (0, n, n_long, h)


def test_fields_bin_and_virtual_offset_of_every_record(program):
    cases = [(w, b) for w, b, _ in ic.good_cases()] + [(w, b) for w, b, _, reason in ic.bad_cases() if reason in (3, 4)]
    streams = [sm.inflate(bam) for _, bam in cases]
    got = _run(program, streams, "good.bin")
    for (what, _), s, g in zip(cases, streams, got):
        assert g == _want(s), what
    assert sum(g[2] for g in got) == 4     # the records beyond 2^29 of the bad cases


def test_a_stream_cut_anywhere_is_refused_without_a_read_past_its_end(program):
    what, bam, _ = ic.good_cases()[[w for w, _, _ in ic.good_cases()].index("CIGARs and flags")]
    stream = sm.inflate(bam)
    _, _, h_end = bm.decode_header(stream)
    bounds, at = {h_end}, h_end
    for r in bm.split_records(stream, h_end):
        at += len(r)
        bounds.add(at)
    cuts = list(range(0, len(stream) + 1))
    got = _run(program, [stream[:k] for k in cuts], "cuts.bin")
    for k, g in zip(cuts, got):
        if k in bounds:
            assert g == _want(stream[:k]), k
        elif k < h_end:
            assert g[0] == -k - 1, k
        else:
            assert g[0] == -max(b for b in bounds if b < k) - 1, k


def test_cigar_words_that_the_record_does_not_hold_are_not_read(program):
    # n_cigar_op says 60 000, the record ends behind two words: the fields come from those two, nothing behind the stream is read
    r = bytearray(ic.rec("short", 0, 100, [(7, "M"), (9, "D")]))
    struct.pack_into("<H", r, 16, 60000)
    from bam_sort_cases import header_bytes
    stream = header_bytes(ic.TEXT, ic.CONTIGS) + bytes(r)
    got, = _run(program, [stream], "short.bin")
    at = len(stream) - len(r)
    v0 = (at // 1000 + (at >= 1000)) << 16 | at % 1000
    assert got == (0, 1, 0, _fnv(2166136261, struct.pack("<QqQQQQQ", at, 0, 100, 116, mi.reg2bin(100, 116), 1, v0)))


def test_sanitizers_were_used_where_the_compiler_has_them(program):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(program[2] / "probe")], input="int main(){}", capture_output=True, text=True)
    assert program[1] == (probe.returncode == 0)
