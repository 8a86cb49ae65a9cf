"""BGZF input for the inflate tests (CPU and GPU share them): families of well-formed blocks, and malformed files made from good blocks
by one targeted edit each.  Everything is made here: Python's zlib plus the BGZF framing, and two small encoders of this module's own
(fixed codes, and dynamic codes with any code lengths) for streams that zlib never writes — a distance of exactly 32 768, a distance
alphabet of a single code, a run of code lengths that crosses from the literal/length lengths into the distance lengths, and the bad
code sets.  zlib's inflate is the judge of every stream made here: good() asserts that it takes the block, and the malformed ones
are asserted to be refused by it (or to fail the CRC32 / ISIZE that it does not see)."""
import struct
import zlib

import numpy as np

Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 1, 2, 3, 4
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def frame(payload, text=None, crc=None, isize=None, bsize=None):
    """one BGZF block round a raw deflate stream"""
    crc = zlib.crc32(text) if crc is None else crc
    isize = len(text) if isize is None else isize
    total = 18 + len(payload) + 8 if bsize is None else bsize
    assert total <= 65536
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", total - 1) + payload + struct.pack("<II", crc, isize)


def deflate(text, level=6, mem=8, strategy=0, flushes=()):
    """raw deflate of text; flushes: (position, zlib flush mode) pairs in its middle"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    out, at = b"", 0
    for pos, mode in flushes:
        out += c.compress(text[at:pos]) + c.flush(mode)
        at = pos
    return out + c.compress(text[at:]) + c.flush()


def block(text, **kw):
    return frame(deflate(text, **kw), text)


def blocks(text, size, **kw):
    return b"".join(block(text[k:k + size], **kw) for k in range(0, len(text), size))


# ---- bit streams of this module's own ----
class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, val, nb):          # nb bits of val, lowest first (header fields, extra bits)
        self.v |= val << self.n
        self.n += nb

    def code(self, c, nb):           # a Huffman code: highest bit first
        for k in range(nb - 1, -1, -1):
            self.put((c >> k) & 1, 1)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canonical(lens):
    """{symbol: (code, length)} of RFC 1951 3.2.2; no check of the set"""
    out, code = {}, 0
    for ln in range(1, 16):
        for s, l in enumerate(lens):
            if l == ln:
                out[s] = (code, ln)
                code += 1
        code <<= 1
    return out


def _len_sym(n):
    base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    extra = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    k = max(i for i in range(29) if base[i] <= n)
    return 257 + k, extra[k], n - base[k]


def _dist_sym(d):
    base = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
    k = max(i for i in range(30) if base[i] <= d)
    return k, max(0, k // 2 - 1), d - base[k]


def _tokens(b, tokens, ll, dd):
    for t in tokens:
        if isinstance(t, tuple):
            s, nb, ex = _len_sym(t[0])
            b.code(*ll[s]); b.put(ex, nb)
            s, nb, ex = _dist_sym(t[1])
            b.code(*dd[s]); b.put(ex, nb)
        else:
            b.code(*ll[t])
    b.code(*ll[256])


def fixed_stream(tokens, final=1):
    """tokens (a byte value, or (length, distance)) as one block with fixed codes"""
    b = Bits()
    b.put(final | 1 << 1, 3)
    _tokens(b, tokens, canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), canonical([5] * 30))
    return b.bytes()


def dynamic_stream(ll_lens, d_lens, tokens, runs=False, final=1):
    """one block with dynamic codes of the given lengths, whatever they are.  The code lengths are sent one by one (code-length symbols
    0 .. 15 of 4 bits each), or with runs=True through symbols 16 / 17 / 18 over the two alphabets' lengths as ONE sequence (0 .. 15 of
    5 bits, 16 / 17 / 18 of 2 / 3 / 3 bits: both code-length codes are complete)."""
    b = Bits()
    b.put(final | 2 << 1, 3)
    b.put(len(ll_lens) - 257, 5); b.put(len(d_lens) - 1, 5); b.put(19 - 4, 4)
    cl_lens = [5] * 16 + [2, 3, 3] if runs else [4] * 16 + [0, 0, 0]
    for s in CL_ORDER:
        b.put(cl_lens[s], 3)
    cl, seq, k = canonical(cl_lens), list(ll_lens) + list(d_lens), 0
    while k < len(seq):
        n = 1
        while k + n < len(seq) and seq[k + n] == seq[k]:
            n += 1
        if runs and seq[k] == 0 and n >= 3:
            n = min(n, 138)
            if n >= 11:
                b.code(*cl[18]); b.put(n - 11, 7)
            else:
                b.code(*cl[17]); b.put(n - 3, 3)
            k += n
        elif runs and n >= 4:
            b.code(*cl[seq[k]])
            n = min(n - 1, 6)
            b.code(*cl[16]); b.put(n - 3, 2)
            k += 1 + n
        else:
            b.code(*cl[seq[k]])
            k += 1
    if tokens is not None:
        _tokens(b, tokens, canonical(ll_lens), canonical(d_lens))
    return b.bytes()


def dynamic_header(payload):
    """(block type, set of code-length symbols used) of the first deflate block of a stream"""
    v = int.from_bytes(payload[:400], "little")
    pos = 0

    def bits(n):
        nonlocal pos
        r = (v >> pos) & ((1 << n) - 1)
        pos += n
        return r
    btype = bits(3) >> 1
    if btype != 2:
        return btype, set()
    hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
    cl_lens = [0] * 19
    for k in range(hclen):
        cl_lens[CL_ORDER[k]] = bits(3)
    table = {(ln, c): s for s, (c, ln) in canonical(cl_lens).items()}
    used, n = set(), 0
    while n < hlit + hdist:
        c, ln = 0, 0
        while (ln, c) not in table:
            c, ln = c << 1 | bits(1), ln + 1
            assert ln <= 7
        s = table[(ln, c)]
        used.add(s)
        n += 1 if s < 16 else 3 + bits(2) if s == 16 else 3 + bits(3) if s == 17 else 11 + bits(7)
    return btype, used


# ---- texts ----
def fastq_text(n_bytes, seed=1):
    rng = np.random.default_rng(seed)
    out, k = [], 0
    while sum(map(len, out)) < n_bytes:
        seq = bytes(rng.choice(list(b"ACGT"), 100).tolist())
        qual = bytes((rng.integers(20, 41, 100) + 33).astype(np.uint8).tolist())
        out.append(b"@read%d/1\n%s\n+\n%s\n" % (k, seq, qual))
        k += 1
    return b"".join(out)[:n_bytes]


def random_bytes(n, seed=2):
    return bytes(np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8).tolist())


_FAMILIES = None


def families():
    """{name: (BGZF bytes, text)}; made once"""
    global _FAMILIES
    if _FAMILIES is not None:
        return _FAMILIES
    F = {}
    fq = fastq_text(9000)
    for level in (1, 6, 9):
        F["level%d" % level] = (blocks(fq, 3000, level=level), fq)
    F["fixed"] = (blocks(fq[:5000], 2500, strategy=Z_FIXED), fq[:5000])
    F["stored"] = (block(fq[:3000], level=0) + block(b"", level=0) + block(fq[3000:4000], level=0), fq[:4000])
    F["huffman_only"] = (block(fq[:4000], strategy=Z_HUFFMAN_ONLY), fq[:4000])
    run = b"N" * 5000
    F["rle"] = (block(run, strategy=Z_RLE), run)
    F["full_flush_twice"] = (block(fq[:6000], flushes=((2000, zlib.Z_FULL_FLUSH), (4000, zlib.Z_FULL_FLUSH))), fq[:6000])
    twice = fq[:1500] + fq[:1500]
    F["sync_flush"] = (block(twice, flushes=((1500, zlib.Z_SYNC_FLUSH),)), twice)
    F["size_1"] = (block(b"x"), b"x")
    big = fastq_text(65536, seed=3)
    F["size_65280"] = (block(big[:65280]), big[:65280])
    F["size_65536"] = (block(big), big)
    rnd = random_bytes(60000)
    F["random"] = (block(rnd), rnd)
    # a repeat at distance exactly 32 768, which zlib never writes (its window stops 262 short): this module's fixed codes
    head = random_bytes(300, seed=5)
    filler = bytes(np.random.default_rng(6).choice(list(b"ACGT"), 32768 - 300).tolist())
    far = head + filler + head
    F["distance_32768"] = (frame(fixed_stream(list(head + filler) + [(258, 32768), (42, 32768)]), far), far)
    far1 = head + filler + b"T" + head
    F["distance_32769"] = (block(far1, level=9), far1)
    small = block(fq[:700])
    F["empty_first_middle_last"] = (EOF_BLOCK + small + block(b"") + small + EOF_BLOCK, fq[:700] * 2)
    F["eof_alone"] = (EOF_BLOCK, b"")
    every = bytes(range(256))
    F["every_byte"] = (block(every), every)
    one = b"A" * 3000
    F["one_value"] = (block(one), one)
    # literal/length: 'A' 1 bit, 256 and 257 (length 3) 2 bits; the distance alphabet is ONE code of one bit (incomplete: zlib takes it)
    ll = [0] * 258
    ll[65], ll[256], ll[257] = 1, 2, 2
    F["single_distance_code"] = (frame(dynamic_stream(ll, [1], [65] + [(3, 1)] * 20), b"A" * 61), b"A" * 61)
    # runs of code lengths through 16 / 17 / 18, one of them across the end of the literal/length lengths: 23 literals from 'a' and
    # 256 .. 264 have 5 bits (a complete code), and so have the distance codes 0 .. 3, so the run of fives goes on into the distance lengths
    ll = [0] * 265
    for s in list(range(97, 97 + 23)) + list(range(256, 265)):
        ll[s] = 5
    dl = [5, 5, 5, 5, 3, 3, 3, 2, 2]
    text = b"abcdefgh" * 3 + b"abc"
    data = dynamic_stream(ll, dl, list(b"abcdefgh") + [(8, 8), (8, 8), (3, 8)], runs=True)
    assert dynamic_header(data)[1] >= {16, 18}
    F["runs_cross_alphabets"] = (frame(data, text), text)
    for name, (data, text) in F.items():
        assert good(data) == text, name
    _FAMILIES = F
    return F


def split(data):
    """[(offset, block bytes)] of well-formed BGZF framing"""
    out, at = [], 0
    while at < len(data):
        n = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append((at, data[at:at + n]))
        at += n
    assert at == len(data)
    return out


def good(data):
    """the text of a BGZF file by zlib, every block's CRC32 and ISIZE checked"""
    text = b""
    for _, blk in split(data):
        t = zlib.decompress(blk[18:-8], -15)
        assert struct.unpack("<II", blk[-8:]) == (zlib.crc32(t), len(t))
        text += t
    return text


def zlib_refuses(payload, isize):
    """does zlib's inflate fail to give exactly isize bytes from this stream?"""
    d = zlib.decompressobj(-15)
    try:
        t = d.decompress(payload, isize + 1)
    except zlib.error:
        return True
    return not (d.eof and len(t) == isize)


_MALFORMED = None


def malformed():
    """{name: (BGZF bytes, offset of the first failing block)}: a good block, the edited one, a good block (where the edit allows it)"""
    global _MALFORMED
    if _MALFORMED is not None:
        return _MALFORMED
    fq = fastq_text(4000, seed=7)
    A = block(fq[:2000])
    G = block(fq[2000:])
    pay, crc, isize = G[18:-8], zlib.crc32(fq[2000:]), 2000
    M = {}

    def put(name, bad, payload=None, size=None):
        if payload is not None:
            assert zlib_refuses(payload, size), name
        M[name] = (A + bad + A, len(A))
    put("truncated_payload", frame(pay[:-10], crc=crc, isize=isize), pay[:-10], isize)
    M["crc_one_bit"] = (A + frame(pay, crc=crc ^ 0x100, isize=isize) + A, len(A))
    put("isize_too_small", frame(pay, crc=crc, isize=isize - 1), pay, isize - 1)
    put("isize_too_large", frame(pay, crc=crc, isize=isize + 1), pay, isize + 1)
    put("btype_3", frame(b"\x07" + pay[1:], crc=crc, isize=isize), b"\x07" + pay[1:], isize)
    st = deflate(fq[:500], level=0)
    assert st[0] == 1 and st[1:3] == struct.pack("<H", 500)
    bad = st[:3] + bytes([st[3] ^ 1]) + st[4:]
    put("stored_len_nlen", frame(bad, fq[:500]), bad, 500)
    ll = [0] * 258
    ll[65], ll[66], ll[256] = 1, 1, 1
    bad = dynamic_stream(ll, [1, 1], [65, 66])
    put("over_subscribed", frame(bad, b"AB"), bad, 2)
    ll = [0] * 258
    ll[65], ll[256] = 2, 2
    bad = dynamic_stream(ll, [1, 1], [65])
    put("incomplete_literal_code", frame(bad, b"A"), bad, 1)
    bad = fixed_stream([65, (3, 2)])
    put("distance_before_start", frame(bad, b"AAAA"), bad, 4)
    M["bsize_past_buffer"] = (A + frame(pay, crc=crc, isize=isize, bsize=18 + len(pay) + 8 + 40), len(A))
    M["garbage_between"] = (A + b"\x55" * 20 + A, len(A))
    _MALFORMED = M
    return M
