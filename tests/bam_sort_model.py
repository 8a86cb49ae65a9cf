"""A plain statement of coordinate-sorted BAM on top of bam_model.py, written from the rule and not from
csrc/bam_sort_util.h: inflate, split the records, sort them stably with Python's sorted by (refID with -1 behind every contig, pos + 1,
the reverse-strand bit), and put SO:coordinate on the header text's @HD line."""
import struct

import bam_model as bm

SO = b"SO:coordinate"


def key(rec, n_ref):
    refid, pos = struct.unpack_from("<ii", rec, 4)
    flag, = struct.unpack_from("<H", rec, 18)
    return (n_ref if refid == -1 else refid, pos + 1, (flag >> 4) & 1)


def packed_key(rec, n_ref):
    """the key in ceil(log2(n_ref + 1)) + 32 + 1 bits, as the radix sort sees it"""
    ref, pos1, rev = key(rec, n_ref)
    return ref << 33 | pos1 << 1 | rev


def key_bits(n_ref):
    return n_ref.bit_length() + 33     # (n_ref.bit_length() = ceil(log2(n_ref + 1)))


def coordinate_text(text):
    lines = text.split(b"\n")
    first = lines[0]
    if first[:3] != b"@HD" or (len(first) > 3 and first[3:4] != b"\t"):
        return b"@HD\tVN:1.6\t" + SO + b"\n" + text
    fields = first.split(b"\t")
    for k in range(1, len(fields)):
        if fields[k][:3] == b"SO:":
            fields[k] = SO
            break
    else:
        fields.append(SO)
    return b"\n".join([b"\t".join(fields)] + lines[1:])


def inflate(bam):
    return b"".join(p for _, p in bm.bgzf_blocks(bam))


def sort_stream(stream):
    """the inflated stream of a BAM file -> (the new header's bytes, the records in coordinate order)"""
    text, contigs, at = bm.decode_header(stream)
    l_text, = struct.unpack_from("<i", stream, 4)
    new_text = coordinate_text(text)
    header = b"BAM\1" + struct.pack("<i", len(new_text)) + new_text + stream[8 + l_text:at]   # (the reference list: the bytes as they were)
    recs = bm.split_records(stream, at)
    n_ref = len(contigs)
    return header, sorted(recs, key=lambda r: key(r, n_ref))


def sort_bam(bam):
    return sort_stream(inflate(bam))


def decode_sorted(bam):
    """a sorted file -> (its header's bytes, its records, the payloads of its blocks); the file must end in the empty block"""
    blocks = bm.bgzf_blocks(bam)
    assert blocks and blocks[-1][1] == b"" and len(blocks[-1][0]) == 28, "no empty end block"
    payloads = [p for _, p in blocks[:-1]]
    stream = b"".join(payloads)
    _, _, at = bm.decode_header(stream)
    return stream[:at], bm.split_records(stream, at), payloads


def check_blocks(header, payloads):
    """the header in blocks of its own, then blocks of whole records of at most 0xff00 bytes, a larger record alone in blocks of its own"""
    at, k = 0, 0
    while at < len(header):
        assert k < len(payloads) and at + len(payloads[k]) <= len(header) and 0 < len(payloads[k]) <= bm.BLOCK, "a header block"
        at += len(payloads[k])
        k += 1
    rest = payloads[k:]
    recs = bm.split_records(b"".join(rest))
    assert [len(p) for p in rest] == bm.cuts(recs)
