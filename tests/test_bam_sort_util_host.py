"""csrc/bam_sort_util.h on the host, through tests/csrc/bam_sort_host_check.cpp (a program of its own: nothing is loaded into Python):
the header's end and rewritten text, every record's offset, size and packed key against tests/bam_sort_model.py, the malformed table
refused at its offsets, and a stream cut anywhere refused without a read past its end.  The program is built with the address and
undefined-behaviour sanitizers where the compiler has their runtimes (every stream is a heap block of its exact size)."""
import os
import struct
import subprocess

import pytest

import bam_model as bm
import bam_sort_cases as sc
import bam_sort_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "bam_sort_host_check.cpp")
INC = os.path.join(ROOT, "mpibwa_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_sort_host")
    exe = str(d / "bam_sort_host_check")
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
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(streams)
    return [(int(c), int(n_ref), int(h_end), int(n), int(a, 16), int(b, 16)) for c, n_ref, h_end, n, a, b in rows]


def _want(stream):
    _, contigs, at = bm.decode_header(stream)
    h_end, n_ref, h, n = at, len(contigs), 2166136261, 0
    for r in bm.split_records(stream, at):
        h = _fnv(h, struct.pack("<QIQ", at, len(r), sm.packed_key(r, n_ref)))
        at += len(r)
        n += 1
    return (0, n_ref, h_end, n, h, _fnv(2166136261, sm.sort_stream(stream)[0]))


def test_header_hop_and_key_of_every_good_case(program):
    streams = [sm.inflate(bam) for _, bam in sc.good_cases()]
    for (what, _), s, got in zip(sc.good_cases(), streams, _run(program, streams, "good.bin")):
        assert got == _want(s), what


def test_the_malformed_table_is_refused_at_its_offsets(program):
    table = []
    for what, bam, code in sc.malformed_cases():
        try:
            table.append((what, sm.inflate(bam), code))
        except Exception:   # the framing's errors (a wrong CRC, a cut block, no BGZF at all): the block table's
            continue
    assert len(table) >= 9
    for (what, _, code), got in zip(table, _run(program, [s for _, s, _ in table], "bad.bin")):
        assert got[0] == code, what


def test_a_stream_cut_anywhere_is_refused_without_a_read_past_its_end(program):
    what, bam = sc.good_cases()[0]
    stream = sm.inflate(bam)
    _, _, h_end = bm.decode_header(stream)
    bounds, at = {h_end}, h_end
    for r in bm.split_records(stream, h_end):
        at += len(r)
        bounds.add(at)
    cuts = list(range(0, h_end + 200)) + list(range(h_end + 200, len(stream), 7))
    got = _run(program, [stream[:k] for k in cuts], "cuts.bin")
    for k, g in zip(cuts, got):
        if k in bounds:
            assert g[0] == 0 and g[2] == h_end, k
        elif k < h_end:
            assert g[0] == -k - 1, k                                  # the header is not complete: the stream's size
        else:
            assert g[0] == -max(b for b in bounds if b < k) - 1, k    # the record that the cut runs through


def test_sanitizers_were_used_where_the_compiler_has_them(program):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(program[2] / "probe")], input="int main(){}", capture_output=True, text=True)
    assert program[1] == (probe.returncode == 0)
