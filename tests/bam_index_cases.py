"""The hand-made inputs of the BAI index for tests/test_bam_index_cases.py (the host path and the model),
tests/test_bam_index_util_host.py (the stand-alone check) and tests/test_gpu_bam_index.py (the device paths): coordinate-sorted BAM files
in blocks chosen here (bam_sort_cases' own_payloads, bam_of and chop), the smallest shapes at which each rule of the index can go wrong.

good_cases() -> [(what, file bytes, designed regions [(ref, beg, end)])], big_case() -> the seeded case of about 200 000 records,
bad_cases() -> [(what, file bytes, code, reason)], unsorted(bam) -> the same records shuffled (seeded), for the fused call."""
import functools
import random
import struct

import bam_model as bm
import bam_sort_cases as sc
import bam_sort_model as sm

CONTIGS = [(b"a", 1 << 29), (b"b", 1_000_000), (b"c", 600_000_000)]
TEXT = b"@HD\tVN:1.6\tSO:coordinate\n@PG\tID:cases\n"
OPS = "MIDNSHP=X"
W = 16384


def rec(name, ref, pos, cigar=(), flag=0, stored_bin=None, pad=0):
    """a record by its fields (pos 0-based, cigar [(length, 'M')]), without SEQ; pad: bytes of a Z tag, to choose its size"""
    name = name.encode() + b"\0"
    words = b"".join(struct.pack("<I", n << 4 | OPS.index(op)) for n, op in cigar)
    if stored_bin is None:
        rlen = sum(n for n, op in cigar if op in "MDN=X") or 1
        stored_bin = bm.reg2bin(max(pos, 0), max(pos, 0) + rlen) & 0xffff
    tag = b"zzZ" + b"p" * (pad - 4) + b"\0" if pad >= 4 else b""
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name), 0, stored_bin, len(cigar), flag, 0, -1, -1, 0) + name + words + tag
    return struct.pack("<i", len(body)) + body


def sort(recs, n_ref=len(CONTIGS)):
    return sorted(recs, key=lambda r: sm.key(r, n_ref))


def file_of(recs, contigs=CONTIGS, eof=True):
    return sc.bam_of(sc.own_payloads(sc.header_bytes(TEXT, contigs), recs), eof)


def file_in_blocks(groups, contigs=CONTIGS, eof=True):
    """the header in a block of its own, then one block per group of records"""
    return sc.bam_of([sc.header_bytes(TEXT, contigs)] + [b"".join(g) for g in groups], eof)


def edges(*positions):
    """the regions around window or record edges: each position +-1"""
    out = []
    for ref, p in positions:
        for lo, hi in ((p - 1, p), (p, p + 1), (p - 1, p + 1), (max(p - W, 0), p), (p, p + W)):
            if 0 <= lo < hi:
                out.append((ref, lo, hi))
    return out


M = lambda n: [(n, "M")]   # noqa: E731


@functools.lru_cache(maxsize=None)
def good_cases():
    out = []
    out.append(("a header only", file_of([]), [(0, 0, 100)]))
    out.append(("only records without a contig", file_of([rec("u%d" % k, -1, -1, flag=4) for k in range(5)]), [(0, 0, 1 << 29), (2, 0, 1000)]))
    three = [rec("x%d" % k, 0, 100 * k, M(50)) for k in range(10)] + [rec("y%d" % k, 2, 5 * W + 7 * k, M(30)) for k in range(10)] + [rec("u", -1, -1, flag=4)]
    out.append(("three contigs, the middle one without records", file_of(three), [(0, 0, 1 << 29), (1, 0, 1_000_000), (2, 0, 1 << 29), (2, 5 * W, 5 * W + 1), (2, 0, 5 * W)]))
    out.append(("pos 0", file_of([rec("p0", 0, 0, M(10)), rec("p1", 0, 0, M(1)), rec("p2", 0, 3, M(4))]), edges((0, 0), (0, 1), (0, 10))))
    out.append(("pos -1 with a contig", file_of([rec("m1", 0, -1, M(10)), rec("m2", 0, -1, (), flag=4), rec("p", 0, 0, M(2))]), edges((0, 0), (0, 10)) + [(0, 0, 1)]))
    out.append(("pos 16383 with 1M: one window, a level-5 bin", file_of([rec("e", 0, W - 1, M(1))]), edges((0, W - 1), (0, W)) + [(0, W, 2 * W)]))
    out.append(("pos 16383 with 2M: two windows, a parent bin", file_of([rec("e", 0, W - 1, M(2))]), edges((0, W - 1), (0, W), (0, W + 1)) + [(0, W, 2 * W)]))
    # a run of bin X, a record across the 16 384 edge (the parent bin), bin X again: the two chunks of X in one block, and a cut between
    x1 = [rec("a%d" % k, 0, W - 200 + 10 * k, M(20)) for k in range(5)]
    span = [rec("s", 0, W - 100, M(300))]
    x2 = [rec("b%d" % k, 0, W - 90 + 10 * k, M(20)) for k in range(5)]
    after = [rec("c%d" % k, 0, W + 500 + k, M(20)) for k in range(3)]
    regions = edges((0, W), (0, W - 100), (0, W + 200)) + [(0, 0, 1 << 29)]
    out.append(("two runs of a bin in one block: joined", file_in_blocks([x1 + span + x2 + after]), regions))
    out.append(("two runs of a bin with a block cut between them: not joined", file_in_blocks([x1 + span, x2 + after]), regions))
    out.append(("the second run begins in the block in which the first, alone in its block, ends: joined", file_in_blocks([x1, span + x2 + after]), regions))
    skip = [rec("n", 0, 1000, [(10, "M"), (500000, "N"), (10, "M")]), rec("in", 0, 200000, M(50)), rec("beh", 0, 501015, M(50))]
    out.append(("10M500000N10M: 31 windows and a high bin", file_of(skip), edges((0, 1000), (0, 501020), (0, 30 * W), (0, 31 * W)) + [(0, 100000, 100100), (0, 200000, 200010), (0, 0, 1 << 29)]))
    gap = [rec("g0", 0, 10, M(20)), rec("g2", 0, 2 * W + 5, M(20)), rec("g5", 0, 5 * W + 5, M(W))]
    out.append(("an empty window between two occupied ones", file_of(gap), edges((0, W), (0, 2 * W), (0, 3 * W), (0, 5 * W)) + [(0, W, 2 * W), (0, 3 * W, 5 * W), (0, 0, 1 << 29)]))
    out.append(("a leading empty window", file_of([rec("l", 1, 3 * W + 1, M(5)), rec("l2", 1, 3 * W + 1, M(5), flag=16)]), edges((1, 3 * W), (1, 3 * W + 1)) + [(1, 0, 3 * W), (1, 0, W)]))
    cf = sort([rec("placed", 0, 5000, (), flag=4 | 1 | 64), rec("f4cig", 0, 5010, M(100), flag=4), rec("ishp", 0, 5020, [(5, "S"), (3, "I"), (2, "H"), (1, "P")]),
               rec("wrongbin", 0, 5030, M(10), stored_bin=1), rec("wrongbin2", 0, 3 * W - 2, M(10), stored_bin=4681), rec("eqx", 0, 5040, [(3, "="), (2, "X"), (4, "D"), (9, "I")])])
    out.append(("CIGARs and flags", file_of(cf), edges((0, 5000), (0, 5001), (0, 5011), (0, 5021), (0, 5049), (0, 3 * W)) + [(0, 5012, 5200)]))
    out.append(("end == 2^29", file_of([rec("last", 0, (1 << 29) - 10, M(10)), rec("last1", 0, (1 << 29) - 1, M(1))]), edges((0, (1 << 29) - 1), (0, (1 << 29) - 10)) + [(0, 0, 1 << 29)]))
    # block layouts
    rng = random.Random(3)
    many = sort([rec("r%04d" % k, rng.choice((0, 0, 2)), rng.randrange(0, 8 * W), M(rng.randrange(1, 200)), flag=rng.choice((0, 16)), pad=rng.randrange(4, 60)) for k in range(400)] +
                [rec("u%d" % k, -1, -1, flag=4) for k in range(3)])
    all_regions = [(0, 0, 1 << 29), (2, 0, 1 << 29)] + edges((0, W), (0, 4 * W), (2, 2 * W))
    header = sc.header_bytes(TEXT, CONTIGS)
    stream = header + b"".join(many)
    out.append(("records that span blocks", sc.bam_of(sc.chop(stream, 1000)), all_regions))
    big = sort(many[:200] + [rec("big", 0, 3 * W, M(10), pad=70000)])
    out.append(("a record that spans two blocks", sc.bam_of(sc.chop(header + b"".join(big), 0xff00)), all_regions))
    p = sc.own_payloads(header, many)
    groups = [many[k:k + 50] for k in range(0, len(many), 50)]
    out.append(("an empty block in the middle", b"".join([sc.block(header), sc.EOF] + [sc.block(b"".join(g)) + sc.EOF for g in groups[:-1]] + [sc.block(b"".join(groups[-1])), sc.EOF]), all_regions))
    out.append(("no end block", file_of(many, eof=False), all_regions))
    out.append(("an empty block and no end block", b"".join([sc.block(header), sc.EOF] + [sc.block(x) for x in p[1:]]), all_regions))
    out.append(("a block cut after every record", file_in_blocks([[r] for r in many]), all_regions))
    for n in (63, 64, 65, 4097):
        recs = sort([rec("k%04d" % k, rng.choice((0, 1, 2)), rng.randrange(0, 40 * W), M(rng.randrange(1, 3000)), flag=rng.choice((0, 16, 4))) for k in range(n)])
        out.append(("%d records" % n, file_of(recs), [(c, 0, 1 << 29) for c in range(3)] + edges((0, 7 * W), (1, 20 * W))))
    return out


def big_records():
    rng = random.Random(17)
    recs = []
    for k in range(200_000):
        kind = rng.random()
        ref, pos = rng.choice((0, 1, 2)), rng.randrange(0, 6_000_000)
        if kind < 0.05:
            cigar = [(50, "M"), (rng.randrange(1, 100_000), "N"), (50, "M")]
        else:
            cigar = [(rng.randrange(20, 151), "M")]
        if kind > 0.975:
            recs.append(rec("q%06d" % k, -1, -1, flag=4))
        elif kind > 0.95:
            recs.append(rec("q%06d" % k, ref, pos, (), flag=4))
        else:
            recs.append(rec("q%06d" % k, ref, pos, cigar, flag=rng.choice((0, 16))))
    return recs


@functools.lru_cache(maxsize=None)
def big_case():
    """about 200 000 records on three contigs, about 5 % with N skips and 5 % unmapped, sorted by the model"""
    return "200 000 seeded records", file_of(sort(big_records())), [(c, 0, 1 << 29) for c in range(3)] + edges((0, 100 * W), (2, 366 * W))


def unsorted(bam, seed=1):
    """the same header and records in a seeded shuffle, in the library's own blocks"""
    stream = sm.inflate(bam)
    _, _, at = bm.decode_header(stream)
    recs = bm.split_records(stream, at)
    random.Random(seed).shuffle(recs)
    return sc.bam_of(sc.own_payloads(stream[:at], recs))


@functools.lru_cache(maxsize=None)
def bad_cases():
    """(what, file, code, reason): beyond 2^29, out of order, a sorted file with the sort's malformed records, and the sort's own table"""
    out = []
    header = sc.header_bytes(TEXT, CONTIGS)
    lead = [rec("a%d" % k, 0, 10 * k, M(5)) for k in range(70)]
    at = len(header) + sum(len(r) for r in lead)
    out.append(("end == 2^29 + 1", file_of(lead + [rec("long", 0, (1 << 29) - 10, M(11))]), -at - 1, 4))
    out.append(("an N skip beyond 2^29", file_of(lead + [rec("long", 0, 1000, [(5, "M"), ((1 << 28) - 1, "N"), ((1 << 28) - 1, "N"), (5, "M")])]), -at - 1, 4))
    out.append(("pos beyond 2^29 on an unmapped read", file_of(lead + [rec("far", 2, 1 << 29, (), flag=4)]), -at - 1, 4))
    second = at + len(rec("x", 0, 900, M(5)))
    out.append(("two records out of order", file_of(lead + [rec("x", 0, 900, M(5)), rec("y", 0, 899, M(5)), rec("z", 0, 2000, M(5))]), -second - 1, 3))
    out.append(("forward behind reverse at one position", file_of(lead + [rec("x", 0, 900, M(5), flag=16), rec("y", 0, 900, M(5))]), -second - 1, 3))
    out.append(("a contig behind the reads without one", file_of(lead + [rec("x", -1, -1, flag=4), rec("yy", 2, 5, M(5))]), -(at + len(rec("x", -1, -1, flag=4))) - 1, 3))
    out.append(("out of order before beyond 2^29", file_of(lead + [rec("x", 0, 900, M(5)), rec("y", 0, 899, M(5)), rec("long", 0, (1 << 29) - 1, M(2))]), -second - 1, 3))
    # the sort's malformed records, in a sorted file
    rng = random.Random(8)
    recs = sort([rec("s%04d" % k, rng.choice((0, 1, 2, -1)), rng.randrange(0, 100000), M(rng.randrange(1, 100)), pad=rng.randrange(4, 300)) for k in range(3000)])
    recs = [r if struct.unpack_from("<i", r, 4)[0] >= 0 else rec("u", -1, -1, flag=4) for r in recs]
    starts, o = [], len(header)
    for r in recs:
        starts.append(o)
        o += len(r)
    sizes = [len(p) for p in sc.own_payloads(header, recs)]

    def patched(k, field_at, value):
        stream = bytearray(header + b"".join(recs))
        struct.pack_into("<i", stream, starts[k] + field_at, value)
        blocks, b = [], 0
        for n in sizes:
            blocks.append(bytes(stream[b:b + n]))
            b += n
        return sc.bam_of(blocks)
    last = len(recs) - 1
    for what, k, field_at, value in (("block_size 31", 400, 0, 31), ("block_size -1", 5, 0, -1), ("a chain that runs past the end", last, 0, len(recs[last]) + 96),
                                     ("refID == n_ref", 300, 4, len(CONTIGS)), ("refID == -2", 301, 4, -2), ("pos == -2", 2650, 8, -2)):
        out.append(("sorted, " + what, patched(k, field_at, value), -starts[k] - 1, 2))
    out.append(("sorted, a last record of three bytes", sc.bam_of(sc.own_payloads(header, recs) + [b"\x20\0\0"]), -o - 1, 2))
    return out
