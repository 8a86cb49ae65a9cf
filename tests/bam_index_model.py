"""A plain statement of the BAI index (SAM specification §5.2) on top of bam_model.py, written from the rules and not from
csrc/bam_index_util.h.

build(bam) -> the index's bytes; parse(bai) -> (contigs, n_no_coor) with contigs = [(bins, ioffset)], bins = {bin: [(beg, end)]};
query(bam, bai, ref, beg, end) -> the records that overlap [beg, end) of contig ref, found through the index as a reader finds them;
scan(bam, ref, beg, end) -> the same by reading every record; Refused(offset, reason) for a file that cannot be indexed."""
import bisect
import functools
import struct

import numpy as np

import bam_model as bm

LIMIT = 1 << 29
PSEUDO = 37450
REF_OPS = (0, 2, 3, 7, 8)     # M D N = X


class Refused(Exception):
    def __init__(self, offset, reason):
        Exception.__init__(self, offset, reason)
        self.offset, self.reason = offset, reason


def interval(rec):
    """(refID, beg, end, mapped) of a record with a contig; (-1, 0, 0, False) of one without"""
    refid, pos, l_name, _mapq, _bin, n_cigar, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    if refid < 0:
        return -1, 0, 0, False
    beg, rlen = max(pos, 0), 0
    for k in range(n_cigar):
        w, = struct.unpack_from("<I", rec, 36 + l_name + 4 * k)
        if w & 15 in REF_OPS:
            rlen += w >> 4
    if flag & 4 or n_cigar == 0 or rlen == 0:
        rlen = 1
    return refid, beg, beg + rlen, not flag & 4


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    """the SAM specification's list of the bins that may hold records overlapping [beg, end)"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


@functools.lru_cache(maxsize=4)
def layout(bam):
    """the file's blocks and records: (n_ref, [(v0, record)], v1 of the last record, [(block's file offset, its payload)])"""
    blocks, at = [], 0
    for raw, payload in bm.bgzf_blocks(bam):
        blocks.append((at, payload))
        at += len(raw)
    stream = b"".join(p for _, p in blocks)
    _, contigs, h_end = bm.decode_header(stream)
    starts, s = [], 0           # (first byte in the stream, file offset) of the blocks that hold bytes
    for off, p in blocks:
        if p:
            starts.append((s, off, len(p)))
        s += len(p)
    recs, k, pos = [], 0, h_end
    for r in bm.split_records(stream, h_end):
        while pos >= starts[k][0] + starts[k][2]:
            k += 1
        recs.append((starts[k][1] << 16 | (pos - starts[k][0]), r))
        pos += len(r)
    behind = 0
    for off, p in blocks:
        if p:
            behind = off + len(bam_block_at(bam, off))
    return len(contigs), recs, behind << 16, blocks


def bam_block_at(bam, off):
    bsize, = struct.unpack_from("<H", bam, off + 16)
    return bam[off:off + bsize + 1]


def check_order(bam):
    """Refused for the first record that sorts before its predecessor or ends beyond 2^29"""
    stream = b"".join(p for _, p in bm.bgzf_blocks(bam))
    _, contigs, at = bm.decode_header(stream)
    n_ref, prev = len(contigs), None
    for r in bm.split_records(stream, at):
        refid, pos = struct.unpack_from("<ii", r, 4)
        flag, = struct.unpack_from("<H", r, 18)
        key = (n_ref if refid == -1 else refid, pos + 1, (flag >> 4) & 1)
        if prev is not None and key < prev:
            raise Refused(at, 3)
        prev = key
        if interval(r)[2] > LIMIT:
            raise Refused(at, 4)
        at += len(r)


def build(bam):
    check_order(bam)
    n_ref, recs, v_end, _ = layout(bam)
    v1 = [v for v, _ in recs[1:]] + [v_end]
    bins = [dict() for _ in range(n_ref)]          # bin -> chunks, in file order
    span = [None] * n_ref                          # [v0 of the first, v1 of the last, mapped, unmapped]
    linear = [[] for _ in range(n_ref)]
    no_coor, last = 0, None
    for (v0, r), end_v in zip(recs, v1):
        refid, beg, end, mapped = interval(r)
        if refid < 0:
            no_coor += 1
            last = None
            continue
        b = reg2bin(beg, end)
        chunks = bins[refid].setdefault(b, [])
        if last == (refid, b):
            chunks[-1][1] = end_v                  # the run goes on
        elif chunks and chunks[-1][1] >> 16 == v0 >> 16:
            chunks[-1][1] = end_v                  # a new run that begins in the block in which the bin's last chunk ends
        else:
            chunks.append([v0, end_v])
        last = (refid, b)
        if span[refid] is None:
            span[refid] = [v0, end_v, 0, 0]
        span[refid][1] = end_v
        span[refid][2 if mapped else 3] += 1
        lin = linear[refid]
        lin.extend([None] * (((end - 1) >> 14) + 1 - len(lin)))
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            if lin[w] is None:
                lin[w] = v0
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for c in range(n_ref):
        out.append(struct.pack("<i", len(bins[c]) + (span[c] is not None)))
        for b in sorted(bins[c]):
            out.append(struct.pack("<Ii", b, len(bins[c][b])))
            out.extend(struct.pack("<QQ", x, y) for x, y in bins[c][b])
        if span[c] is not None:
            out.append(struct.pack("<IiQQQQ", PSEUDO, 2, *span[c]))
        out.append(struct.pack("<i", len(linear[c])))
        prev = 0
        for v in linear[c]:
            prev = prev if v is None else v
            out.append(struct.pack("<Q", prev))
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


@functools.lru_cache(maxsize=4)
def parse(bai):
    assert bai[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", bai, 4)
    at, contigs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", bai, at)
        at += 4
        bins, order = {}, []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, at)
            at += 8
            assert b not in bins
            bins[b] = [struct.unpack_from("<QQ", bai, at + 16 * k) for k in range(n_chunk)]
            order.append(b)
            at += 16 * n_chunk
        assert order == sorted(x for x in order if x != PSEUDO) + [PSEUDO] * (PSEUDO in bins)
        n_intv, = struct.unpack_from("<i", bai, at)
        at += 4
        ioffset = list(struct.unpack_from("<%dQ" % n_intv, bai, at))
        at += 8 * n_intv
        contigs.append((bins, ioffset))
    no_coor, = struct.unpack_from("<Q", bai, at)
    assert at + 8 == len(bai)
    return contigs, no_coor


def _read_from(order, payloads, v, v_end):
    """the records from virtual offset v up to v_end: seek to the block, skip `within` bytes, read on across blocks"""
    k, within, out = bisect.bisect_left(order, v >> 16), v & 0xffff, []
    assert order[k] == v >> 16, "a virtual offset that names no block"
    while True:
        while k < len(order) and within >= len(payloads[k]):   # the next block that holds the byte
            within -= len(payloads[k])
            k += 1
        if k == len(order) or (order[k] << 16 | within) >= v_end:
            return out
        if within + 4 <= len(payloads[k]):   # a record that its block holds whole: no copy of the block's rest
            size = 4 + struct.unpack_from("<i", payloads[k], within)[0]
            if within + size <= len(payloads[k]):
                out.append(payloads[k][within:within + size])
                within += size
                continue
        data, j = payloads[k][within:], k
        while len(data) < 4 or len(data) < 4 + struct.unpack_from("<i", data, 0)[0]:   # the record goes on in the next blocks
            j += 1
            data += payloads[j]
        size = 4 + struct.unpack_from("<i", data, 0)[0]
        out.append(data[:size])
        within += size


def query(bam, bai, ref, beg, end):
    """as the specification's reader: the chunks of reg2bins' bins, without those that end at or before the window's ioffset"""
    contigs, _ = parse(bai)
    bins, ioffset = contigs[ref]
    _, _, _, blocks = layout(bam)
    order, payloads = [off for off, _ in blocks], [p for _, p in blocks]
    w = beg >> 14
    low = ioffset[w] if w < len(ioffset) else (ioffset[-1] if ioffset else 0)
    chunks = sorted(c for b in reg2bins(beg, end) if b in bins and b != PSEUDO for c in bins[b] if c[1] > low)
    out, seen_to = [], 0
    for c_beg, c_end in chunks:
        c_beg = max(c_beg, seen_to)
        if c_beg >= c_end:
            continue
        for r in _read_from(order, payloads, c_beg, c_end):
            refid, r_beg, r_end, _ = interval(r)
            if refid == ref and r_beg < end and r_end > beg:
                out.append(r)
        seen_to = c_end
    return out


@functools.lru_cache(maxsize=4)
def _intervals(bam):
    recs = [r for _, r in layout(bam)[1]]
    spans = np.array([interval(r)[:3] for r in recs], dtype=np.int64).reshape(-1, 3)
    return recs, spans


def scan(bam, ref, beg, end):
    """the brute-force answer: every record of the file against the region"""
    recs, s = _intervals(bam)
    return [recs[k] for k in np.nonzero((s[:, 0] == ref) & (s[:, 1] < end) & (s[:, 2] > beg))[0]]
