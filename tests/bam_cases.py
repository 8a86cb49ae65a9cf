"""The hand-made table of edges for the BAM encoders (tests/test_bam_cases.py on the host, tests/test_gpu_bam.py on the device): SAM
lines built field by field, a contig table that needs no index, and the calls through ctypes."""
import ctypes as C

# (the second "chr1" is never found: the first of equal names counts)
CONTIGS = [(b"chr1", 250_000_000), (b"chr2", 200_000_000), (b"chr10", 1000), (b"chr1_KI270706v1_alt", 5000), (b"chr1", 7), (b"c", 12)]
NAMES = [n for n, _ in CONTIGS]


class fake_bns:
    """a bntseq_t with CONTIGS, kept alive with its strings"""
    def __init__(self):
        from mpibwa_amd import abi
        self.anns = (abi.bntann1_t * len(CONTIGS))()
        for i, (name, length) in enumerate(CONTIGS):
            self.anns[i].name = name
            self.anns[i].anno = b""
            self.anns[i].len = length
        self.bns = abi.bntseq_t()
        self.bns.n_seqs = len(CONTIGS)
        self.bns.anns = self.anns
        self.bns.l_pac = sum(l for _, l in CONTIGS)
        self.ptr = C.pointer(self.bns)


def line(qname=b"read1", flag=99, rname=b"chr1", pos=1000, mapq=60, cigar=b"10M", rnext=b"=", pnext=1200, tlen=210, seq=b"ACGTACGTAC", qual=b"IIIIIHHHH#",
         tags=()):
    def num(v):
        return v if isinstance(v, bytes) else b"%d" % v
    return b"\t".join([qname, num(flag), rname, num(pos), num(mapq), cigar, rnext, num(pnext), num(tlen), seq, qual] + list(tags))


FLOATS = [b"0.5", b"-0.5", b"+1.25", b"3.141593", b"0.000001", b"123456789.654321", b"-0.0", b"16777217.0", b"16777219.5", b"999999999.999999",
          b"0.1", b"0.333333", b"1e-3", b"-2.5E+3", b"7", b".5", b"6.02e23", b"1.17549435e-38", b"1e-45"]


def good_lines():
    """(what, line): every edge a well-formed line can stand on"""
    out = []
    bases = b"ACGTNacgtnRYKMSWBDHV=.-*"
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129):
        seq = bytes(bases[k % len(bases)] for k in range(n)) or b"*"
        qual = bytes(33 + (k * 7) % 60 for k in range(n)) or b"*"
        out.append(("l_seq %d" % n, line(seq=seq, qual=qual, cigar=b"%dM" % n if n else b"*")))
        if n:
            out.append(("l_seq %d, QUAL *" % n, line(seq=seq, qual=b"*", cigar=b"*")))
    out.append(("QNAME of 1 byte", line(qname=b"q")))
    out.append(("QNAME of 254 bytes", line(qname=b"n" * 254)))
    out.append(("CIGAR *", line(cigar=b"*")))
    out.append(("every operation", line(cigar=b"1M2I3D4N5S6H7P8=9X", seq=b"ACGTA" * 5, qual=b"F" * 25)))
    out.append(("a length of 2^28 - 1", line(cigar=b"268435455N3M", seq=b"ACG", qual=b"III")))
    out.append(("a length of 2^28 - 1, soft clip", line(cigar=b"268435455S")))
    out.append(("POS 0", line(pos=0, rname=b"*", cigar=b"*", flag=4)))
    out.append(("POS 0 on a contig", line(pos=0)))
    for k in (14, 17, 20, 23, 26):
        edge = 1 << k
        out.append(("a span that ends at the %d boundary" % edge, line(pos=edge - 9, cigar=b"10M")))      # pos0 = edge - 10 .. edge - 1
        out.append(("a span that crosses the %d boundary" % edge, line(pos=edge - 8, cigar=b"10M")))      # .. edge
        out.append(("a span that starts at the %d boundary" % edge, line(pos=edge + 1, cigar=b"10M")))
        out.append(("a deletion across the %d boundary" % edge, line(pos=edge - 3, cigar=b"2M5D3M2I3M")))
    out.append(("a span across 2^29", line(pos=(1 << 29) - 2, cigar=b"10M")))
    out.append(("the largest POS", line(pos=2 ** 31 - 1, pnext=2 ** 31 - 1)))
    out.append(("RNEXT =", line(rnext=b"=")))
    out.append(("RNEXT *", line(rnext=b"*", pnext=0)))
    out.append(("RNEXT another contig", line(rnext=b"chr2")))
    out.append(("RNEXT the same contig by name", line(rnext=b"chr1")))
    out.append(("RNAME *, RNEXT =", line(rname=b"*", rnext=b"=", flag=77, pos=0, cigar=b"*")))
    out.append(("a contig whose name is a prefix of others", line(rname=b"c", rnext=b"chr10")))
    out.append(("the ALT contig", line(rname=b"chr1_KI270706v1_alt", rnext=b"chr10")))
    out.append(("negative TLEN", line(tlen=-210)))
    out.append(("TLEN at both ends", line(tlen=-2 ** 31, tags=[b"NM:i:0"])))
    out.append(("TLEN at the top", line(tlen=2 ** 31 - 1)))
    out.append(("FLAG and MAPQ at the top", line(flag=65535, mapq=255)))
    out.append(("no tags", line()))
    for v in (-2 ** 31, -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 2 ** 32 - 1):
        out.append(("i %d" % v, line(tags=[b"NM:i:%d" % v, b"AS:i:%d" % v])))
    out.append(("i with a plus sign", line(tags=[b"XS:i:+17", b"X0:i:-0"])))
    out.append(("an empty Z", line(tags=[b"MD:Z:", b"NM:i:1"])))
    out.append(("an empty Z last", line(tags=[b"NM:i:1", b"MD:Z:"])))
    out.append(("Z with : , ;", line(tags=[b"SA:Z:chr2,100,+,5S5M,60,0;chr1,7,-,5M5S,0,1;", b"XA:Z:chr10,-12,10M,0;", b"RG:Z:a:b:c", b"MC:Z:10M", b"MQ:i:60", b"ms:i:350"])))
    out.append(("A tags", line(tags=[b"XT:A:U", b"xx:A::", b"yy:A:\x7f"])))
    out.append(("pa:f", line(tags=[b"NM:i:0", b"pa:f:0.987", b"AS:i:10"])))
    out.append(("an H tag", line(tags=[b"hh:H:1AE301", b"NM:i:3"])))
    out.append(("an empty H tag", line(tags=[b"hh:H:"])))
    out.append(("B tags", line(tags=[b"b1:B:c,-128,127,0", b"b2:B:C,255", b"b3:B:s,-32768,32767", b"b4:B:S,65535,0", b"b5:B:i,-2147483648,2147483647",
                                     b"b6:B:I,4294967295", b"b7:B:f,0.5,-1.25,1e3", b"b8:B:c", b"NM:i:2"])))
    out.append(("floats of every form", line(tags=[b"f" + bytes([97 + k]) + b":f:" + t for k, t in enumerate(FLOATS)])))
    out.append(("a quality below 33 wraps as a byte", line(seq=b"AC", qual=b" ~", cigar=b"2M")))
    return out


def bad_lines():
    """(what, line): every malformed line; none of them ends the process"""
    out = [("an empty line", b""),
           ("one field", b"only"),
           ("ten fields", b"\t".join(line().split(b"\t")[:10])),
           ("an empty field", line(cigar=b"")),
           ("an RNAME the table does not have", line(rname=b"chr3")),
           ("an RNAME that is a prefix of a name", line(rname=b"chr")),
           ("an RNAME that is a name and more", line(rname=b"chr11")),
           ("an RNEXT the table does not have", line(rnext=b"chrZ")),
           ("a non-digit in FLAG", line(flag=b"9x")),
           ("a sign in FLAG", line(flag=b"-1")),
           ("FLAG above 65535", line(flag=65536)),
           ("a non-digit in POS", line(pos=b"10 0")),
           ("POS above 2^31 - 1", line(pos=2 ** 31)),
           ("a non-digit in MAPQ", line(mapq=b"6O")),
           ("MAPQ above 255", line(mapq=256)),
           ("a non-digit in PNEXT", line(pnext=b"1e3")),
           ("a non-digit in TLEN", line(tlen=b"--3")),
           ("TLEN below -2^31", line(tlen=-2 ** 31 - 1)),
           ("TLEN above 2^31 - 1", line(tlen=2 ** 31)),
           ("a CIGAR operation that is none", line(cigar=b"10Q")),
           ("a CIGAR without a length", line(cigar=b"M")),
           ("a CIGAR that ends in digits", line(cigar=b"10M5")),
           ("a CIGAR length of 2^28", line(cigar=b"268435456M")),
           ("QUAL shorter than SEQ", line(qual=b"IIIIIHHHH")),
           ("QUAL longer than SEQ", line(qual=b"IIIIIHHHH##")),
           ("QUAL beside SEQ *", line(seq=b"*", qual=b"II", cigar=b"*")),
           ("a QNAME of 255 bytes", line(qname=b"n" * 255)),
           ("a tab at the end", line() + b"\t"),
           ("an empty tag", line(tags=[b"", b"NM:i:1"])),
           ("a short tag", line(tags=[b"NM:i"])),
           ("a tag without its colons", line(tags=[b"NM-i-1"])),
           ("a tag type that is none", line(tags=[b"NM:q:1"])),
           ("an A of two bytes", line(tags=[b"XT:A:UU"])),
           ("an empty i", line(tags=[b"NM:i:"])),
           ("a non-digit in i", line(tags=[b"NM:i:1O"])),
           ("an f that is no number", line(tags=[b"pa:f:0.5x"])),
           ("a B of an unknown subtype", line(tags=[b"bb:B:q,1"])),
           ("a B element outside its type", line(tags=[b"bb:B:c,128"])),
           ("an empty B element", line(tags=[b"bb:B:c,,1"]))]
    for v in (-2 ** 31 - 1, 2 ** 32, 10 ** 19, -10 ** 19, 10 ** 25):
        out.append(("i %d" % v, line(tags=[b"NM:i:%d" % v])))
    return out


def growth_lines():
    """(what, line): the lines whose record is larger than their text"""
    few = dict(qname=b"q", flag=0, rname=b"c", pos=1, mapq=0, rnext=b"*", pnext=0, tlen=0)
    return [("fixed fields of one byte", line(cigar=b"*", seq=b"*", qual=b"*", **few)),
            ("CIGAR operations of two text bytes", line(cigar=b"1M1I" * 500, seq=b"*", qual=b"*", **few)),
            ("QUAL * beside a long SEQ", line(cigar=b"*", seq=b"ACGT" * 250, qual=b"*", **few)),
            ("QUAL * beside an odd SEQ", line(cigar=b"*", seq=b"ACGTA" * 201, qual=b"*", **few)),
            ("B elements of two text bytes", line(cigar=b"*", seq=b"*", qual=b"*", tags=[b"bb:B:i" + b",1" * 800, b"bf:B:f" + b",2" * 800], **few)),
            ("many B tags without elements", line(cigar=b"*", seq=b"*", qual=b"*", tags=[b"b%d:B:c" % (k % 10) for k in range(40)], **few)),
            ("all of them", line(cigar=b"1M" * 300, seq=b"A" * 301, qual=b"*", tags=[b"bb:B:I" + b",7" * 300], **few))]


def line_of_record_size(size):
    """a line whose record has exactly `size` bytes (30 000 of them SEQ and QUAL, the rest a Z tag)"""
    pad = size - (36 + 2 + 10000 + 20000 + 4)
    assert pad >= 0
    return line(qname=b"b", cigar=b"*", seq=b"C" * 20000, qual=b"*", tags=[b"zz:Z:" + b"p" * pad])


def many_lines(rng, n, device_only=False):
    """n lines of the program's kind with random lengths: what a chunk looks like, in small"""
    out = []
    for k in range(n):
        l = int(rng.integers(1, 300))
        seq = bytes(rng.choice(list(b"ACGTN"), l).tolist())
        qual = bytes((rng.integers(2, 42, l) + 33).astype("uint8").tolist())
        contig = NAMES[int(rng.integers(0, 4))]
        tags = [b"NM:i:%d" % rng.integers(0, 9), b"MD:Z:%d" % l, b"AS:i:%d" % rng.integers(-5, 300), b"XS:i:%d" % rng.integers(0, 70000)]
        if k % 5 == 0:
            tags.append(b"pa:f:%.3f" % rng.random())
        if k % 7 == 0:
            tags.append(b"XA:Z:chr2,-%d,%dM,1;" % (rng.integers(1, 10 ** 8), l))
        if k % 11 == 0 and not device_only:
            tags.append(b"bb:B:s,1,2,-3")
        out.append(line(qname=b"r%d" % k, flag=int(rng.integers(0, 4096)), rname=contig, pos=int(rng.integers(0, 2 ** 28)), mapq=int(rng.integers(0, 61)),
                        cigar=b"%dM" % l, rnext=(b"=", b"*", b"chr2")[k % 3], pnext=int(rng.integers(0, 2 ** 28)), tlen=int(rng.integers(-900, 900)),
                        seq=seq, qual=qual if k % 13 else b"*", tags=tags))
    return b"".join(ln + b"\n" for ln in out)


def host_records(lib, bns, text):
    cap = lib.mi355x_bam_bound(len(text))
    out = C.create_string_buffer(max(cap, 1))
    n = C.c_int64(-1)
    size = lib.mi355x_sam_to_bam(text, len(text), bns.ptr, out, cap, C.byref(n))
    assert size >= 0, size
    return out.raw[:size], n.value


def host_compress(lib, bns, text, level):
    cap = lib.mi355x_bgzf_bound(lib.mi355x_bam_bound(len(text)))
    out = C.create_string_buffer(cap)
    size = lib.mi355x_bam_compress(text, len(text), bns.ptr, level, out, cap)
    assert size >= 0, size
    return out.raw[:size]
