"""The device BAM encoder (csrc/bam_kernel.hip, csrc/bam_stage.hip): mi355x_sam_to_bam_dev gives the bytes of
mi355x_sam_to_bam and of tests/bam_model.py on bam_cases.py's table of edges and on the SAM the library writes for the example data;
mi355x_bam_compress_dev gives well-formed BGZF blocks of whole records, cut where the host cuts, the same bytes on every call and from
four threads at once, over one and over three pieces, without a buffer growing after a context's first call."""
import ctypes as C
import gzip
import os
import tarfile
import threading

import numpy as np
import pytest

import bam_cases as bc
import bam_model as bm

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EX = os.path.join(HERE, "golden", "mpibwa_examples")


@pytest.fixture(scope="module")
def lib(built):
    from mpibwa_amd import api
    return api.load_library()


@pytest.fixture(scope="module")
def bns():
    return bc.fake_bns()


def _counts(lib):
    c = (C.c_uint64 * 6)()
    lib.mi355x_bam_dev_counts(c)
    return list(c)


def _dev_records(lib, bns_ptr, text):
    cap = lib.mi355x_bam_bound(len(text))
    out = C.create_string_buffer(max(cap, 1))
    n = C.c_int64(-1)
    size = lib.mi355x_sam_to_bam_dev(text, len(text), bns_ptr, out, cap, C.byref(n))
    return (out.raw[:size], n.value) if size >= 0 else (size, 0)


def _host_records(lib, bns_ptr, text):
    cap = lib.mi355x_bam_bound(len(text))
    out = C.create_string_buffer(max(cap, 1))
    n = C.c_int64(-1)
    size = lib.mi355x_sam_to_bam(text, len(text), bns_ptr, out, cap, C.byref(n))
    return (out.raw[:size], n.value) if size >= 0 else (size, 0)


def _dev_compress(lib, bns_ptr, text, cap=None):
    cap = lib.mi355x_bgzf_bound(lib.mi355x_bam_bound(len(text))) if cap is None else cap
    out = C.create_string_buffer(max(cap, 1))
    size = lib.mi355x_bam_compress_dev(text, len(text), bns_ptr, out, cap)
    return out.raw[:size] if size >= 0 else size


@pytest.fixture(scope="module")
def example(tmp_path_factory, lib):
    """(engine, SAM text): what the library writes for the first 1 500 pairs of the example data, with the FASTQ's own qualities"""
    from mpibwa_amd import abi, api
    d = tmp_path_factory.mktemp("bamex")
    with tarfile.open(os.path.join(EX, "hg19.small.tar.gz")) as t:
        t.extractall(d)
    mates = []
    for k in (1, 2):
        with gzip.open(os.path.join(EX, "HCC1187C_R%d_10K.fastq.gz" % k), "rb") as g:
            lines = g.read().split(b"\n")
        mates.append([(lines[i][1:].split()[0], lines[i + 1], lines[i + 3]) for i in range(0, 4 * 1500, 4)])
    reads, quals = [], {}
    for (n1, s1, q1), (n2, s2, q2) in zip(*mates):
        name = n1[:-2] if n1.endswith(b"/1") else n1
        reads.append((name, s1, s2))
        quals[name] = (q1, q2)
    eng = api.Engine(os.path.join(str(d), "hg19.small.fa"), device=0)
    sam = b"".join(eng.process(eng.opt(flag=abi.MEM_F_PE), reads))
    out = []
    for ln in sam.split(b"\n")[:-1]:
        f = ln.split(b"\t")
        if f[10] != b"*":
            q = quals[f[0]][1 if int(f[1]) & 0x80 else 0]
            if int(f[1]) & 0x10:
                q = q[::-1]
            if len(q) == len(f[10]):   # (a hard-clipped line keeps its own)
                f[10] = q
        out.append(b"\t".join(f))
    text = b"".join(ln + b"\n" for ln in out)
    assert len(out) >= 3000
    return eng, text


def test_the_table_of_edges(lib, bns):
    # what the device encodes itself, in one text; then every line alone, the two that it declines included
    own = [ln for what, ln in bc.good_lines() if what not in ("B tags", "floats of every form")]
    c0 = _counts(lib)
    text = b"".join(ln + b"\n" for ln in own)
    want, n = bm.encode(text, bc.NAMES)
    assert _dev_records(lib, bns.ptr, text) == (want, n) == _host_records(lib, bns.ptr, text)
    c1 = _counts(lib)
    assert c1[0] - c0[0] == n and c1[1] == c0[1] and c1[2] - c0[2] == len(text) and c1[3] - c0[3] == len(want)   # none of them went to the host
    for what, ln in bc.good_lines():
        assert _dev_records(lib, bns.ptr, ln + b"\n") == (bm.encode_record(ln, bc.NAMES), 1), what
    floats = b"".join(bc.line(tags=[b"pa:f:%.3f" % (k / 1000.0)]) + b"\n" for k in range(1001))
    c1 = _counts(lib)
    assert _dev_records(lib, bns.ptr, floats)[0] == bm.encode(floats, bc.NAMES)[0]
    assert _counts(lib)[1] == c1[1]
    assert _dev_records(lib, bns.ptr, b"") == (b"", 0)


def test_lines_of_63_64_65_bytes_and_a_tab_at_a_windows_end(lib, bns):
    lines = []
    for total in (63, 64, 65, 127, 128, 129, 64, 64, 63, 65):   # with the newline
        base = bc.line(qname=b"q", seq=b"ACGT", qual=b"IIII", cigar=b"4M", tags=[b"MD:Z:"])
        lines.append(base + b"p" * (total - 1 - len(base)))
    text = b"".join(ln + b"\n" for ln in lines)
    assert [len(ln) + 1 for ln in lines] == [63, 64, 65, 127, 128, 129, 64, 64, 63, 65]
    assert _dev_records(lib, bns.ptr, text) == bm.encode(text, bc.NAMES)
    # every field's tab in turn as byte 63 of a 64-byte window
    for field in range(11):
        ln = bc.line(tags=[b"NM:i:1"])
        at = len(b"\t".join(ln.split(b"\t")[:field + 1]))          # the tab behind the field, in the line
        pad = bc.line(qname=b"p", tags=[b"MD:Z:" + b"x" * ((63 - at - len(bc.line(qname=b"p", tags=[b"MD:Z:"])) - 1) % 64)])
        text = pad + b"\n" + ln + b"\n"
        assert text[len(pad) + 1 + at] == 9 and (len(pad) + 1 + at) % 64 == 63
        assert _dev_records(lib, bns.ptr, text) == bm.encode(text, bc.NAMES)
    # a newline as the last byte of a window and of a 4-KiB chunk, and many short lines
    short = bc.line(qname=b"q", flag=4, rname=b"*", pos=0, mapq=0, cigar=b"*", rnext=b"*", pnext=0, tlen=0, seq=b"*", qual=b"*") + b"\n"
    text = short * 3000 + bc.many_lines(np.random.default_rng(1), 300, device_only=True) + short * 7
    assert _dev_records(lib, bns.ptr, text) == bm.encode(text, bc.NAMES)


def test_a_declined_line_in_the_middle_moves_the_counter(lib, bns):
    rng = np.random.default_rng(2)
    own = bc.many_lines(rng, 400, device_only=True)
    for what, ln in (("a B tag", bc.line(tags=[b"bb:B:c,1,2"])), ("an exponent", bc.line(tags=[b"xf:f:1e-3"])),
                     ("a record above 0xff00 bytes", bc.line(seq=b"A" * 50000, qual=b"I" * 50000))):
        text = own + ln + b"\n" + own
        c0 = _counts(lib)
        want, n = bm.encode(text, bc.NAMES)
        assert _dev_records(lib, bns.ptr, text) == (want, n), what
        c1 = _counts(lib)
        assert c1[1] - c0[1] == n == c1[0] - c0[0], what
        z = _dev_compress(lib, bns.ptr, text)
        assert b"".join(p for _, p in bm.bgzf_blocks(z)) == want, what
        assert [len(p) for _, p in bm.bgzf_blocks(z)] == bm.cuts(bm.split_records(want)), what


def test_malformed_lines_return_the_hosts_code(lib, bns):
    ok = bc.line()
    own = bc.many_lines(np.random.default_rng(3), 100, device_only=True)
    for what, bad in bc.bad_lines():
        text = own + bad + b"\n" + ok + b"\n"
        want = -len(own) - 1
        assert _host_records(lib, bns.ptr, text)[0] == want, what
        assert _dev_records(lib, bns.ptr, text)[0] == want, what
    text = own + bc.bad_lines()[4][1] + b"\n"
    assert _dev_compress(lib, bns.ptr, text) == -len(own) - 1
    for text, want in ((ok, -1), (own + ok, -len(own) - 1), (b"x\n" + own + ok, -1)):
        assert _dev_records(lib, bns.ptr, text)[0] == want == _host_records(lib, bns.ptr, text)[0]
        assert _dev_compress(lib, bns.ptr, text) == want


def test_the_example_datas_sam(lib, example):
    eng, text = example
    names = [eng.bns.contents.anns[i].name for i in range(eng.bns.contents.n_seqs)]
    want, n = bm.encode(text, names)
    c0 = _counts(lib)
    assert _dev_records(lib, eng.bns, text) == (want, n) == _host_records(lib, eng.bns, text)
    assert _counts(lib)[1] == c0[1]
    lines = text.split(b"\n")[:-1]
    assert [bm.decode_record(r, names) for r in bm.split_records(want)] == [bm.normalise(ln) for ln in lines]
    one = lines[5] + b"\n"
    assert _dev_records(lib, eng.bns, one) == (bm.encode_record(lines[5], names), 1)


def test_blocks_of_whole_records(lib, example):
    eng, text = example
    names = [eng.bns.contents.anns[i].name for i in range(eng.bns.contents.n_seqs)]
    recs = bm.split_records(bm.encode(text, names)[0])
    c0 = _counts(lib)
    z = _dev_compress(lib, eng.bns, text)
    blocks = bm.bgzf_blocks(z)
    assert b"".join(p for _, p in blocks) == b"".join(recs)
    assert [len(p) for _, p in blocks] == bm.cuts(recs) and len(blocks) > 10
    for _, p in blocks:
        assert b"".join(bm.split_records(p)) == p
    c1 = _counts(lib)
    assert [c1[k] - c0[k] for k in range(6)] == [len(recs), 0, len(text), sum(len(r) for r in recs), len(blocks), len(z)]
    assert len(z) < 0.7 * len(text)
    # the host path cuts where the device cuts
    cap = lib.mi355x_bgzf_bound(lib.mi355x_bam_bound(len(text)))
    out = C.create_string_buffer(cap)
    hsize = lib.mi355x_bam_compress(text, len(text), eng.bns, 1, out, cap)
    hz = out.raw[:hsize]
    assert [p for _, p in bm.bgzf_blocks(hz)] == [p for _, p in blocks]
    # a second call: the same bytes, no buffer grows
    g0 = lib.mi355x_buffer_growths()
    assert _dev_compress(lib, eng.bns, text) == z
    assert lib.mi355x_buffer_growths() == g0
    # four threads at once
    got = [None] * 4

    def work(k):
        got[k] = _dev_compress(lib, eng.bns, text)
    th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert all(g == z for g in got)
    # cap too small
    assert _dev_compress(lib, eng.bns, text, cap=65536) == b""
    assert _dev_compress(lib, eng.bns, b"") == b""


def test_one_text_over_three_pieces(example, tmp_path):
    """tests/bam_three_pieces.py, in a process of its own (it holds a few hundred MB of buffers)"""
    import json
    import subprocess
    import sys
    eng, text = example
    bns = eng.bns.contents
    (tmp_path / "text.sam").write_bytes(text)
    (tmp_path / "contigs.json").write_text(json.dumps([(bns.anns[i].name.decode(), bns.anns[i].len) for i in range(bns.n_seqs)]))
    r = subprocess.run([sys.executable, os.path.join(HERE, "bam_three_pieces.py"), str(tmp_path / "text.sam"), str(tmp_path / "contigs.json")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "three pieces:" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
