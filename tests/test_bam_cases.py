"""The host BAM encoder (csrc/bam_util.h, csrc/sampost.cpp) against tests/bam_model.py, byte for byte: mi355x_sam_to_bam,
mi355x_bam_header, mi355x_bam_bound, mi355x_bam_compress.  CPU only, through ctypes.

The inputs are bam_cases.py's hand-made table of edges (always) and the reference's SAM for pairs of every kind under -M, -a, -Y, -C, a
read group and an ALT genome (where oracle/_ref is built)."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import bam_cases as bc
import bam_model as bm
from oracle import pyoracle as po


@pytest.fixture(scope="module")
def lib(built):
    from mpibwa_amd import api
    return api.load_library()


def test_the_library_the_binding_and_the_header_declare_the_entry_points(lib):
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    head = re.sub(r"\s+", " ", open(os.path.join(root, "include", "mpibwa_amd.h")).read())
    for decl in ("int64_t mi355x_bam_header(const char *text, size_t len, const bntseq_t *bns, uint8_t *out, size_t cap);",
                 "int64_t mi355x_bam_bound(size_t sam_len);",
                 "int64_t mi355x_sam_to_bam(const char *sam, size_t len, const bntseq_t *bns, uint8_t *out, size_t cap, int64_t *n_records);",
                 "int64_t mi355x_sam_to_bam_dev(const char *sam, size_t len, const bntseq_t *bns, uint8_t *out, size_t cap, int64_t *n_records);",
                 "int64_t mi355x_bam_compress(const char *sam, size_t len, const bntseq_t *bns, int level, uint8_t *out, size_t cap);",
                 "int64_t mi355x_bam_compress_dev(const char *sam, size_t len, const bntseq_t *bns, uint8_t *out, size_t cap);",
                 "void mi355x_bam_dev_counts(uint64_t out[6]);"):
        assert decl in head
        assert getattr(lib, decl.split("(")[0].split()[-1]).argtypes is not None
    c = (C.c_uint64 * 6)()
    lib.mi355x_bam_dev_counts(c)   # (host code: counts since load)
    assert c[0] >= c[1]


def test_header(lib):
    bns = bc.fake_bns()
    for text in (b"", b"@HD\tVN:1.6\n", b"@SQ\tSN:chr1\tLN:5\n@PG\tID:x\tCL:a b\tc\n"):
        want = bm.encode_header(text, bc.CONTIGS)
        out = C.create_string_buffer(len(want))
        assert lib.mi355x_bam_header(text, len(text), bns.ptr, out, len(want)) == len(want)
        assert out.raw == want
        assert bm.decode_header(want) == (text, bc.CONTIGS, len(want))
        assert lib.mi355x_bam_header(text, len(text), bns.ptr, out, len(want) - 1) == 0


def test_every_edge_of_the_table_alone_and_together(lib):
    bns = bc.fake_bns()
    good = []
    for what, line in bc.good_lines():
        want = bm.encode_record(line, bc.NAMES)
        got, n = bc.host_records(lib, bns, line + b"\n")
        assert got == want and n == 1, what
        assert bm.normalise(line) == bm.decode_record(got, bc.NAMES), what
        assert len(want) <= lib.mi355x_bam_bound(len(line) + 1), what
        good.append(line)
    text = b"".join(ln + b"\n" for ln in good)
    want, n = bm.encode(text, bc.NAMES)
    got, got_n = bc.host_records(lib, bns, text)
    assert got == want and got_n == n == len(good)
    assert [bm.decode_record(r, bc.NAMES) for r in bm.split_records(got)] == [bm.normalise(ln) for ln in good]
    assert bc.host_records(lib, bns, b"") == (b"", 0)
    # cap: one byte short gives 0
    out = C.create_string_buffer(len(want))
    assert lib.mi355x_sam_to_bam(text, len(text), bns.ptr, out, len(want) - 1, None) == 0
    # what the table covers
    lens = {int(struct.unpack_from("<i", r, 20)[0]) for r in bm.split_records(got)}
    assert {0, 1, 2, 63, 64, 65, 127, 128, 129} <= lens
    assert 4680 in {struct.unpack_from("<H", r, 14)[0] for r in bm.split_records(got)}


def test_the_float_division_is_exact_at_all_1001_values(lib):
    bns = bc.fake_bns()
    lines = [bc.line(tags=[b"pa:f:%.3f" % (k / 1000.0)]) for k in range(1001)] + [bc.line(tags=[b"xf:f:" + t]) for t in bc.FLOATS]
    text = b"".join(ln + b"\n" for ln in lines)
    got, n = bc.host_records(lib, bns, text)
    want, _ = bm.encode(text, bc.NAMES)
    assert got == want and n == len(lines)
    # the model's rounding itself, against numpy's float32 on values a double holds exactly enough
    for t in (b"0.333", b"0.1", b"16777217.0", b"0.000001", b"999999999999.999999", b"1e-3", b"-2.5E+3"):
        assert bm.float32_bits(t) == int(np.float32(float(t)).view(np.uint32)), t
    assert bm.float32_bits(b"16777217.0") == 0x4b800000 and bm.float32_bits(b"16777219.0") == 0x4b800002   # ties to even, both ways
    assert bm.float32_bits(b"-0.000") == 0x80000000


def test_malformed_lines_give_their_offset(lib):
    bns = bc.fake_bns()
    ok = bc.line()
    for what, bad in bc.bad_lines():
        for before in (0, 1, 3):
            text = (ok + b"\n") * before + bad + b"\n" + ok + b"\n"
            want = -before * (len(ok) + 1) - 1
            assert bm.encode(text, bc.NAMES)[0] == want, what
            out = C.create_string_buffer(lib.mi355x_bam_bound(len(text)))
            assert lib.mi355x_sam_to_bam(text, len(text), bns.ptr, out, len(out), None) == want, what
            zcap = lib.mi355x_bgzf_bound(lib.mi355x_bam_bound(len(text)))
            assert lib.mi355x_bam_compress(text, len(text), bns.ptr, 6, C.create_string_buffer(zcap), zcap) == want, what
    # a last line without its newline, alone and behind good lines; an earlier malformed line wins
    for text, want in ((ok, -1), (ok + b"\n" + ok, -len(ok) - 2), (b"x\n" + ok, -1)):
        assert bm.encode(text, bc.NAMES)[0] == want
        out = C.create_string_buffer(lib.mi355x_bam_bound(len(text)))
        assert lib.mi355x_sam_to_bam(text, len(text), bns.ptr, out, len(out), None) == want


def test_the_bound_holds_at_the_growth_cases(lib):
    bns = bc.fake_bns()
    for what, line in bc.growth_lines():
        text = line + b"\n"
        got, _ = bc.host_records(lib, bns, text)
        assert got == bm.encode_record(line, bc.NAMES), what
        assert len(text) < len(got) <= lib.mi355x_bam_bound(len(text)), what   # (they do grow, and the bound holds)
    assert lib.mi355x_bam_bound(0) >= 0
    # many minimal lines: 16 bytes of growth per line
    text = bc.line(qname=b"q", rname=b"*", pos=0, mapq=0, cigar=b"*", rnext=b"*", pnext=0, tlen=0, seq=b"*", qual=b"*", flag=4) + b"\n"
    assert len(text) == 22
    got, n = bc.host_records(lib, bns, text * 1000)
    assert n == 1000 and len(got) == 38 * 1000 <= lib.mi355x_bam_bound(22 * 1000)


def test_many_segments_give_the_same_bytes_from_1_and_16_threads(lib):
    """The host encoder works in segments of 4 MB of whole lines: a text of three segments and a bit, on 1 and on 16 threads, against the
    model; then a malformed line in the third segment, one in the second and the third (the earlier one is reported), and a last line
    without its newline behind three good segments."""
    bns = bc.fake_bns()
    part = bc.many_lines(np.random.default_rng(5), 1500)
    text = part * ((13 << 20) // len(part) + 1)
    assert 12 << 20 < len(text) < 16 << 20
    want, n = bm.encode(part, bc.NAMES)
    reps = len(text) // len(part)
    bad = bc.line(rname=b"chr3") + b"\n"
    at2, at3 = text.index(b"\n", 5 << 20) + 1, text.index(b"\n", 9 << 20) + 1   # line starts in the second and in the third segment
    outs = []
    for threads in ("1", "16"):
        os.environ["MPIBWA_SAMPOST_THREADS"] = threads
        try:
            got, got_n = bc.host_records(lib, bns, text)
            assert got_n == n * reps and got == want * reps
            outs.append(bc.host_compress(lib, bns, text, 1))
            out = C.create_string_buffer(lib.mi355x_bam_bound(len(text) + 2 * len(bad)))
            for t, code in ((text[:at3] + bad + text[at3:], -at3 - 1), (text[:at2] + bad + text[at2:at3] + bad + text[at3:], -at2 - 1),
                            (text + bc.line(), -len(text) - 1), (text[:at3] + bad + text[at3:] + bc.line(), -at3 - 1)):
                assert lib.mi355x_sam_to_bam(t, len(t), bns.ptr, out, len(out), None) == code
        finally:
            os.environ.pop("MPIBWA_SAMPOST_THREADS", None)
    assert outs[0] == outs[1]
    payloads = [p for _, p in bm.bgzf_blocks(outs[0])]
    assert b"".join(payloads) == want * reps and [len(p) for p in payloads] == bm.cuts(bm.split_records(want) * reps)


def test_blocks_hold_whole_records(lib):
    bns = bc.fake_bns()
    rng = np.random.default_rng(3)
    text = bc.many_lines(rng, 1500)
    recs = bm.split_records(bm.encode(text, bc.NAMES)[0])
    outs = {}
    for threads in ("1", "16"):
        os.environ["MPIBWA_SAMPOST_THREADS"] = threads
        try:
            for level in (1, 6):
                outs[threads, level] = bc.host_compress(lib, bns, text, level)
            assert bc.host_records(lib, bns, text)[0] == b"".join(recs)
        finally:
            os.environ.pop("MPIBWA_SAMPOST_THREADS", None)
    assert outs["1", 1] == outs["16", 1] and outs["1", 6] == outs["16", 6]
    payloads = [p for _, p in bm.bgzf_blocks(outs["1", 6])]
    assert b"".join(payloads) == b"".join(recs)
    assert [len(p) for p in payloads] == bm.cuts(recs) and len(payloads) > 5
    for p in payloads:
        assert b"".join(bm.split_records(p)) == p   # the block_size chain ends at the payload's end
    # a block of exactly 0xff00 bytes, and a record a byte over
    a = bc.line(qname=b"a", seq=b"A" * 1000, qual=b"I" * 1000)
    la = len(bm.encode_record(a, bc.NAMES))
    fill = 0xff00 - la
    for extra, want in ((0, [0xff00, la]), (1, [la, fill + 1, la])):
        b = bc.line_of_record_size(fill + extra)
        assert len(bm.encode_record(b, bc.NAMES)) == fill + extra
        text = b"".join(x + b"\n" for x in (a, b, a))
        z = bc.host_compress(lib, bns, text, 6)
        assert [len(p) for _, p in bm.bgzf_blocks(z)] == want == bm.cuts(bm.split_records(bm.encode(text, bc.NAMES)[0]))
    # a record larger than a block is cut into full blocks; the stream is still the records
    big = bc.line(qname=b"big", seq=b"G" * 100000, qual=b"J" * 100000)
    text = b"".join(x + b"\n" for x in (a, big, a))
    z = bc.host_compress(lib, bns, text, 1)
    pl = [p for _, p in bm.bgzf_blocks(z)]
    assert b"".join(pl) == bm.encode(text, bc.NAMES)[0] and [len(p) for p in pl] == bm.cuts(bm.split_records(b"".join(pl)))
    # cap too small: 0
    assert lib.mi355x_bam_compress(text, len(text), bns.ptr, 6, C.create_string_buffer(65536), 65536) == 0
    assert bc.host_compress(lib, bns, b"", 6) == b""


def test_the_references_sam_of_every_option(genome, genome_alt, lib):
    if not po.ref_available():
        pytest.skip("oracle/_ref/libbwaref.so not built")
    from mpibwa_amd import abi, simulate
    from test_sampost import _pairs_of_every_kind, _with_qualities
    rng = np.random.default_rng(12)
    seen = set()
    for g in (genome, genome_alt):
        ref = po.RefIndex(g["prefix"])
        names = [n.encode() for n in g["names"]]
        reads = simulate.reads_to_ascii(_pairs_of_every_kind(g, n=120, seed=6))
        runs = [(dict(flag=abi.MEM_F_PE), None, None), (dict(flag=abi.MEM_F_PE | abi.MEM_F_NO_MULTI), None, None), (dict(flag=abi.MEM_F_PE | abi.MEM_F_ALL), None, None),
                (dict(flag=abi.MEM_F_PE | abi.MEM_F_SOFTCLIP), None, None), (dict(flag=abi.MEM_F_PE), "BC:Z:ACGT-TT;x,y:z\tq1:i:-77\tq2:A:!\tq3:f:0.25", None),
                (dict(flag=abi.MEM_F_PE), None, "@RG\\tID:grp1\\tSM:s"), (dict(), None, None)]
        for kw, comment, rg in runs:
            ref.set_rg(rg)
            try:
                rd = reads if kw.get("flag", 0) & abi.MEM_F_PE else [(n, a, None) for n, a, _ in reads]
                text = _with_qualities(b"".join(ref.process(ref.opt(**kw), rd, comment=comment)), rng)
            finally:
                ref.set_rg(None)
            want, n = bm.encode(text, names)
            assert n == text.count(b"\n") and n >= len(rd)
            out = C.create_string_buffer(lib.mi355x_bam_bound(len(text)))
            nrec = C.c_int64(0)
            size = lib.mi355x_sam_to_bam(text, len(text), ref.bns, out, len(out), C.byref(nrec))
            assert size == len(want) and out.raw[:size] == want and nrec.value == n
            lines = text.split(b"\n")[:-1]
            assert [bm.decode_record(r, names) for r in bm.split_records(want)] == [bm.normalise(ln) for ln in lines]
            for ln in lines:
                seen.update(t[:4] for t in ln.split(b"\t")[11:])
    assert {b"NM:i", b"MD:Z", b"AS:i", b"XS:i", b"SA:Z", b"XA:Z", b"RG:Z", b"pa:f", b"BC:Z", b"q1:i", b"q2:A", b"q3:f"} <= seen, seen
