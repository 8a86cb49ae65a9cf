"""The hand-made inputs of the BAM sort for tests/test_bam_sort_cases.py (the host path), tests/test_gpu_bam_sort.py
(the device path) and tests/test_gpu_bam_sort_program.py: BAM files built from bam_cases.line() / bam_model.encode in BGZF blocks
written here with zlib, in the library's own layout (the header in blocks of its own, blocks of whole records) and in foreign ones.

good_cases() -> [(what, file bytes)], piece_case() -> the one case with more output blocks than a device piece holds, many_case() ->
the one case with enough records for the host path's chunks and merges and enough input blocks for more than two inflate groups,
malformed_cases() -> [(what, file bytes, the code both paths must return)]."""
import functools
import random
import struct
import zlib

import bam_cases as bc
import bam_model as bm

EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
TEXT = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:250000000\n@PG\tID:mpibwa\n"


def block(payload, level=1):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    z = c.compress(payload) + c.flush()
    assert len(payload) <= 0x10000 and len(z) + 26 <= 0x10000
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(z) + 25) + z +
            struct.pack("<II", zlib.crc32(payload), len(payload)))


def _gzip(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def chop(data, n=bm.BLOCK):
    return [data[k:k + n] for k in range(0, len(data), n)]


def own_payloads(header, recs):
    """the library's own layout: the header in blocks of its own, then blocks of whole records"""
    out, at = chop(header), 0
    body = b"".join(recs)
    for n in bm.cuts(recs):
        out.append(body[at:at + n])
        at += n
    return out


def bam_of(payloads, eof=True):
    return b"".join(block(p) for p in payloads) + (EOF if eof else b"")


def records(lines, names=bc.NAMES):
    data, n = bm.encode(b"".join(ln + b"\n" for ln in lines), names)
    assert n == len(lines)
    return bm.split_records(data)


def header_bytes(text, contigs):
    """bam_model.encode_header's bytes, joined once (the table of 70 000 contigs)"""
    refs = b"".join(struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", l) for n, l in contigs)
    return b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(contigs)) + refs


def own(lines, text=TEXT, contigs=bc.CONTIGS, eof=True):
    return bam_of(own_payloads(header_bytes(text, contigs), records(lines, [n for n, _ in contigs])), eof)


def needs_host_walk(bam):
    """does a block that holds records start or end inside a record? (then the device leaves the walk to the host)"""
    payloads = [p for _, p in bm.bgzf_blocks(bam)]
    stream = b"".join(payloads)
    _, _, at = bm.decode_header(stream)
    h_end, bounds = at, {at}
    for r in bm.split_records(stream, at):
        at += len(r)
        bounds.add(at)
    end = 0
    for p in payloads:
        end += len(p)
        if end > h_end and end not in bounds:
            return True
    return False


def mixed_lines(rng, n):
    """n lines over every contig, unmapped ones among them, with names that tell the input order"""
    out = []
    for k in range(n):
        kind = rng.randrange(8)
        name = b"r%05d" % k
        if kind == 0:
            out.append(bc.line(qname=name, flag=77, rname=b"*", pos=0, mapq=0, cigar=b"*", rnext=b"*", pnext=0, tlen=0))
        elif kind == 1:   # an unmapped read that carries its mate's coordinates: it sorts there
            out.append(bc.line(qname=name, flag=69, rname=b"chr2", pos=rng.randrange(1, 5000), mapq=0, cigar=b"*", rnext=b"=", pnext=7, tlen=0))
        else:
            contig = bc.NAMES[rng.choice((0, 1, 2, 3, 5))]
            out.append(bc.line(qname=name, flag=rng.choice((99, 147, 83, 163, 0, 16)), rname=contig, pos=rng.randrange(1, 900), rnext=b"="))
    return out


@functools.lru_cache(maxsize=None)
def good_cases():
    rng = random.Random(5)
    out = []
    # ties: one contig and position, forward and reverse; 10 000 records with one key and distinct names
    ties = [bc.line(qname=b"t%d" % k, flag=(16 if k % 3 == 0 else 0), rname=b"chr2", pos=700) for k in range(40)] + mixed_lines(rng, 30)
    out.append(("ties, forward and reverse", own(ties)))
    out.append(("10 000 records with one key", own([bc.line(qname=b"n%d" % k, flag=0, rname=b"chr10", pos=5, seq=b"AC", qual=b"II", cigar=b"2M") for k in range(10000)])))
    # unmapped reads among mapped ones
    out.append(("unmapped reads among mapped ones", own(mixed_lines(rng, 400))))
    # edge positions: POS 0 (pos -1) and 1 (pos 0), the largest POS, the first and the last contig
    edges = [bc.line(qname=b"e%d" % k, rname=r, pos=p, pnext=1, cigar=b"*", flag=f)
             for k, (r, p, f) in enumerate([(b"c", 2 ** 31 - 1, 0), (b"chr1", 2 ** 31 - 1, 16), (b"c", 1, 16), (b"chr1", 1, 0), (b"chr1", 0, 0), (b"c", 0, 16),
                                            (b"*", 0, 4), (b"*", 2 ** 31 - 1, 4), (b"chr1", 2 ** 31 - 1, 0), (b"c", 1, 0)])]
    out.append(("edge positions", own(edges)))
    # key widths
    for n_ref in (1, 2, 3, 255, 256, 70000):
        contigs = [(b"k%d" % k, 1000 + k) for k in range(n_ref)]
        names = sorted({0, n_ref // 2, n_ref - 1})
        lines = [bc.line(qname=b"w%d" % j, rname=b"chr1", pos=1 + (7 * j) % 5, flag=(16 if j % 2 else 0), rnext=b"*", pnext=0, tlen=0) for j in range(12)]
        lines.insert(3, bc.line(qname=b"u", flag=4, rname=b"*", pos=0, cigar=b"*", rnext=b"*", pnext=0, tlen=0))
        recs = [bytearray(r) for r in records(lines)]
        for j, r in enumerate(recs):   # (the contig by its number: no table of 70 000 names for the encoder)
            if j != 3:
                struct.pack_into("<i", r, 4, names[j % len(names)])
        out.append(("n_ref %d" % n_ref, bam_of(own_payloads(header_bytes(TEXT, contigs), [bytes(r) for r in recs]))))
    # counts
    for n in (0, 1, 63, 64, 65):
        out.append(("%d records" % n, own(mixed_lines(rng, n))))
    # orders
    up = [bc.line(qname=b"o%d" % k, rname=b"chr1", pos=10 + k) for k in range(300)]
    out.append(("already sorted", own(up)))
    out.append(("reverse sorted", own(up[::-1])))
    # alignments: record sizes and starts at every offset modulo 16
    out.append(("QNAME lengths 1 to 17", own([bc.line(qname=b"q" * (1 + k % 17), rname=bc.NAMES[k % 3], pos=1 + (k * 37) % 101) for k in range(170)])))
    # large records: at the block size, one byte under, one byte above, and one of three blocks (the last two are cut across blocks)
    big = [bc.line_of_record_size(s) for s in (0xfeff, 0xff00, 0xff01, 140000)]
    out.append(("large records", own(mixed_lines(rng, 5) + big[:2] + mixed_lines(rng, 5) + big[2:] + mixed_lines(rng, 3))))
    # foreign layouts
    lines = mixed_lines(rng, 3000)
    header, recs = bm.encode_header(TEXT, bc.CONTIGS), records(lines)
    stream = header + b"".join(recs)
    out.append(("cut every 0xff00 bytes", bam_of(chop(stream))))
    out.append(("cut every 1000 bytes", bam_of(chop(stream, 1000))))
    mid = own_payloads(b"", recs)
    out.append(("a header that ends mid-block", bam_of([header + mid[0]] + mid[1:])))
    out.append(("no empty end block", own(lines, eof=False)))
    p = own_payloads(header, recs)
    out.append(("empty blocks in the middle", b"".join([EOF, block(p[0]), EOF, EOF] + [block(x) + EOF for x in p[1:]])))
    # header texts
    for what, text in (("no @HD", b"@SQ\tSN:chr1\tLN:250000000\n"), ("@HD VN:1.5", b"@HD\tVN:1.5\n@SQ\tSN:chr1\tLN:250000000\n"),
                       ("SO:unsorted GO:query", b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n@CO\tSO:unsorted stays\n"), ("SO:coordinate already", b"@HD\tVN:1.6\tSO:coordinate\n"),
                       ("an empty text", b""), ("@HD without a newline", b"@HD\tVN:1.6"), ("a first line that only begins like @HD", b"@HDX\tVN:1.6\n")):
        out.append(("header text: " + what, own(mixed_lines(rng, 20), text=text)))
    return out


@functools.lru_cache(maxsize=None)
def piece_case():
    """more output blocks than a device piece holds (512): about 35 MB of records of about 1 000 bytes, made from one record"""
    rng = random.Random(9)
    rec = bytearray(records([bc.line(qname=b"piece0000000", rname=b"chr1", pos=1, cigar=b"600M", seq=b"ACGT" * 150, qual=b"F" * 600, tags=[b"NM:i:0", b"MD:Z:600"])])[0])
    recs = []
    for k in range(36000):
        pos = rng.randrange(0, 200_000_000)
        struct.pack_into("<ii", rec, 4, rng.choice((0, 1, -1)), pos)
        struct.pack_into("<H", rec, 14, bm.reg2bin(pos, pos + 600) & 0xffff)
        struct.pack_into("<H", rec, 18, rng.choice((0, 16)))
        rec[36:48] = b"piece%07d" % k
        recs.append(bytes(rec))
    return "more blocks than a piece", bam_of(own_payloads(bm.encode_header(TEXT, bc.CONTIGS), recs))


@functools.lru_cache(maxsize=None)
def many_case():
    """70 001 small records (above the 65 536 at which the host path sorts in 64 chunks and merges them; 70 001 = 64 * 1 093 + 49, so
    the chunks have two sizes) with 30 distinct keys and names that tell the input order, in blocks of 40 whole records: 1 751 input
    blocks, more than two of the device's inflate groups of 512"""
    rng = random.Random(11)
    rec = bytearray(records([bc.line(qname=b"m0000000", flag=0, rname=b"chr1", pos=1, cigar=b"2M", seq=b"AC", qual=b"II", rnext=b"*", pnext=0, tlen=0)])[0])
    recs = []
    for k in range(70001):
        pos = rng.choice((0, 7, 8, 4000, 2 ** 31 - 2))
        struct.pack_into("<ii", rec, 4, rng.choice((0, 2, -1)), pos)
        struct.pack_into("<H", rec, 14, bm.reg2bin(pos, pos + 2) & 0xffff)
        struct.pack_into("<H", rec, 18, rng.choice((0, 16)))
        rec[36:44] = b"m%07d" % k
        recs.append(bytes(rec))
    blocks = [b"".join(recs[k:k + 40]) for k in range(0, len(recs), 40)]
    return "65 536 records and more, 1 751 input blocks", bam_of(chop(bm.encode_header(TEXT, bc.CONTIGS)) + blocks)


@functools.lru_cache(maxsize=None)
def malformed_cases():
    rng = random.Random(6)
    lines = mixed_lines(rng, 3000)
    last = len(lines) - 1
    header, recs = bm.encode_header(TEXT, bc.CONTIGS), records(lines)
    n_ref = len(bc.CONTIGS)
    starts, at = [], len(header)
    for r in recs:
        starts.append(at)
        at += len(r)
    sizes = [len(p) for p in own_payloads(header, recs)]

    def patched(k, field_at, fmt, value):
        """record k with one field replaced, in the blocks the good file has"""
        stream = bytearray(header + b"".join(recs))
        struct.pack_into(fmt, stream, starts[k] + field_at, value)
        out, o = [], 0
        for n in sizes:
            out.append(bytes(stream[o:o + n]))
            o += n
        return bam_of(out)
    out = [("block_size 31", patched(400, 0, "<i", 31), -starts[400] - 1),
           ("block_size -1", patched(5, 0, "<i", -1), -starts[5] - 1),
           ("a chain that runs past the end", patched(last, 0, "<i", len(recs[last]) - 4 + 100), -starts[last] - 1),
           ("a last record of three bytes", bam_of(own_payloads(header, recs) + [b"\x20\0\0"]), -at - 1),
           ("refID == n_ref", patched(300, 4, "<i", n_ref), -starts[300] - 1),
           ("refID == -2", patched(301, 4, "<i", -2), -starts[301] - 1),
           ("pos == -2", patched(2650, 8, "<i", -2), -starts[2650] - 1)]
    good = own(lines)
    blocks = [b for b, _ in bm.bgzf_blocks(good)]
    assert len(blocks) >= 4
    second = len(blocks[0]) + len(blocks[1])
    crc_at = second + len(blocks[2]) - 8
    out.append(("a block with a wrong CRC", good[:crc_at] + bytes([good[crc_at] ^ 1]) + good[crc_at + 1:], -second - 1))
    out.append(("a first block that is not BAM\\1", bam_of(own_payloads(b"BAM\2" + header[4:], recs)), -1))
    no_eof = good[:-28]
    out.append(("a truncated last block", no_eof[:-7], -(len(no_eof) - len(blocks[-2])) - 1))
    both = bam_of(own_payloads(b"BAM\2" + header[4:], recs), eof=False)
    out.append(("a bad header and a truncated last block: the block's code", both[:-7], -(len(both) - len(bm.bgzf_blocks(both)[-1][0])) - 1))
    out.append(("a header cut off by the end of the file", bam_of([header[:-3]]), -(len(header) - 3) - 1))
    out.append(("plain gzip", _gzip(b"@HD\tVN:1.6\n"), -1))
    out.append(("SAM text", b"@HD\tVN:1.6\n" + lines[0] + b"\n", -1))
    out.append(("an empty file", b"", -1))
    return out


def example_bam(lib, bns_ptr, text):
    """what `mpibwa_gpu --bam --device-bgzf` writes for a chunk's SAM text: the binary header in zlib's blocks, the chunk's records from
    mi355x_bam_compress_dev, the empty end block"""
    import ctypes as C
    bns = bns_ptr.contents
    head_text = b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (bns.anns[i].name, bns.anns[i].len) for i in range(bns.n_seqs)) + b"@PG\tID:mpibwa_amd\tPN:mpibwa_amd\n"
    cap = len(head_text) + 64 * (bns.n_seqs + 1)
    raw = C.create_string_buffer(cap)
    n = lib.mi355x_bam_header(head_text, len(head_text), bns_ptr, raw, cap)
    assert n > 0
    zcap = lib.mi355x_bgzf_bound(n)
    z = C.create_string_buffer(zcap)
    hn = lib.mi355x_bgzf_compress(raw.raw[:n], n, 3, z, zcap)
    assert hn > 0
    cap = lib.mi355x_bgzf_bound(lib.mi355x_bam_bound(len(text)))
    out = C.create_string_buffer(cap)
    size = lib.mi355x_bam_compress_dev(text, len(text), bns_ptr, out, cap)
    assert size > 0
    return z.raw[:hn] + out.raw[:size] + EOF
