"""A plain statement of the BAM layout: an encoder and a decoder in Python, written from the layout and not from
csrc/bam_util.h, for tests/test_bam_cases.py, tests/test_gpu_bam.py and tests/test_gpu_bam_driver.py.

Everything is little-endian.  A record: int32 block_size (the bytes that follow), int32 refID, int32 pos (POS - 1), uint8 l_read_name
(with the NUL), uint8 mapq, uint16 bin, uint16 n_cigar_op, uint16 flag, int32 l_seq, int32 next_refID, int32 next_pos, int32 tlen, QNAME NUL,
CIGAR words (len << 4 | op), SEQ two bases per byte, QUAL - 33 (0xff: '*'), tags.  A float is rounded to float32 exactly: the two
neighbours of the decimal value are compared as fractions, no double stands on the way."""
import struct
from fractions import Fraction

CIGAR_OPS = "MIDNSHP=X"
SEQ_CODES = "=ACMGRSVTWYHKDBN"
BLOCK = 0xff00


class Malformed(Exception):
    pass


def _uint(text, top):
    if not text or any(c not in b"0123456789" for c in text) or len(text) > 19:
        raise Malformed(text)
    v = int(text)
    if v > top:
        raise Malformed(text)
    return v


def _int(text, low, top):
    body = text[1:] if text[:1] in (b"-", b"+") else text
    if not body or any(c not in b"0123456789" for c in body) or len(body) > 19:
        raise Malformed(text)
    v = int(text)
    if not low <= v <= top:
        raise Malformed(text)
    return v


def float32_bits(text):
    """the bits of the float32 nearest to the decimal text (ties to even); text: sign, digits, '.', digits, an optional exponent"""
    t = text.decode()
    try:
        x = Fraction(t)
    except (ValueError, ZeroDivisionError):
        raise Malformed(text)
    if t.strip() != t or "_" in t or "/" in t:
        raise Malformed(text)
    sign = 0x80000000 if t.startswith("-") else 0
    x = abs(x)
    if x == 0:
        return sign
    # the largest e with 2^e <= x, then the 24-bit integer mantissa by floor and a comparison of the remainder with one half
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    e = max(e, -126)                      # (below: subnormal, the mantissa has no hidden bit)
    scaled = x / Fraction(2) ** (e - 23)  # in [2^23, 2^24) for a normal number
    m = scaled.numerator // scaled.denominator
    rest = scaled - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m & 1):
        m += 1
    if m == 1 << 24:
        m >>= 1
        e += 1
    if e > 127:
        return sign | 0x7f800000
    if m < 1 << 23:                       # subnormal
        return sign | m
    return sign | (e + 127) << 23 | (m & 0x7fffff)


def reg2bin(beg, end):
    end -= 1
    for k in (14, 17, 20, 23, 26):
        if beg >> k == end >> k:          # (Python's >> is arithmetic)
            return ((1 << (29 - k)) - 1) // 7 + (beg >> k)
    return 0


def _int_tag(v):
    if v >= 0:
        for letter, fmt, top in (("C", "<B", 255), ("S", "<H", 65535), ("I", "<I", 2 ** 32 - 1)):
            if v <= top:
                return letter.encode() + struct.pack(fmt, v)
    else:
        for letter, fmt, low in (("c", "<b", -128), ("s", "<h", -32768), ("i", "<i", -2 ** 31)):
            if v >= low:
                return letter.encode() + struct.pack(fmt, v)
    raise Malformed(v)


_ARRAY = {"c": ("<b", -128, 127), "C": ("<B", 0, 255), "s": ("<h", -32768, 32767), "S": ("<H", 0, 65535),
          "i": ("<i", -2 ** 31, 2 ** 31 - 1), "I": ("<I", 0, 2 ** 32 - 1)}


def encode_tag(tag):
    if len(tag) < 5 or tag[2:3] != b":" or tag[4:5] != b":":
        raise Malformed(tag)
    name, kind, val = tag[:2], tag[3:4], tag[5:]
    if kind == b"A":
        if len(val) != 1:
            raise Malformed(tag)
        return name + b"A" + val
    if kind == b"i":
        return name + _int_tag(_int(val, -2 ** 31, 2 ** 32 - 1))
    if kind == b"f":
        return name + b"f" + struct.pack("<I", float32_bits(val))
    if kind in (b"Z", b"H"):
        return name + kind + val + b"\0"
    if kind == b"B":
        parts = val.split(b",")
        sub = parts[0].decode()
        if sub == "f":
            body = b"".join(struct.pack("<I", float32_bits(p)) for p in parts[1:])
        elif sub in _ARRAY:
            fmt, low, top = _ARRAY[sub]
            body = b"".join(struct.pack(fmt, _int(p, low, top)) for p in parts[1:])
        else:
            raise Malformed(tag)
        return name + b"B" + sub.encode() + struct.pack("<i", len(parts) - 1) + body
    raise Malformed(tag)


def encode_record(line, names):
    """line: one SAM line without its newline; names: the contigs in order (the first of equal names counts)"""
    f = line.split(b"\t")
    if len(f) < 11 or any(not x for x in f):
        raise Malformed(line)
    index = {}
    for i, n in enumerate(names):
        index.setdefault(n, i)

    def ref(name, same):
        if name == b"*":
            return -1
        if same is not None and name == b"=":
            return same
        if name not in index:
            raise Malformed(name)
        return index[name]
    qname = f[0]
    if len(qname) > 254:
        raise Malformed(qname)
    flag = _uint(f[1], 65535)
    refid = ref(f[2], None)
    pos = _uint(f[3], 2 ** 31 - 1) - 1
    mapq = _uint(f[4], 255)
    ops, ref_len = [], 0
    if f[5] != b"*":
        num = b""
        for c in f[5]:
            ch = bytes([c])
            if ch.isdigit():
                num += ch
                continue
            if not num or ch.decode("latin1") not in CIGAR_OPS or int(num) > 2 ** 28 - 1:
                raise Malformed(f[5])
            op = CIGAR_OPS.index(ch.decode())
            ops.append(int(num) << 4 | op)
            if ch in b"MDN=X":
                ref_len += int(num)
            num = b""
        if num or len(ops) > 65535:
            raise Malformed(f[5])
    next_refid = ref(f[6], refid)
    next_pos = _uint(f[7], 2 ** 31 - 1) - 1
    tlen = _int(f[8], -2 ** 31, 2 ** 31 - 1)
    seq = b"" if f[9] == b"*" else f[9]
    if f[10] == b"*":
        qual = b"\xff" * len(seq)
    else:
        if len(f[10]) != len(seq):
            raise Malformed(f[10])
        qual = bytes((c - 33) & 0xff for c in f[10])
    codes = [SEQ_CODES.index(chr(c).upper()) if chr(c).upper() in SEQ_CODES and (chr(c) == "=" or chr(c).isalpha()) else 15 for c in seq]
    if len(codes) & 1:
        codes.append(0)
    packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2))
    end = pos + (ref_len if ref_len else 1)
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(qname) + 1, mapq, reg2bin(pos, end) & 0xffff, len(ops), flag, len(seq), next_refid, next_pos, tlen)
    body += qname + b"\0" + b"".join(struct.pack("<I", w) for w in ops) + packed + qual + b"".join(encode_tag(t) for t in f[11:])
    return struct.pack("<i", len(body)) + body


def encode(sam, names):
    """the records of the SAM text back to back and their number, or the error code -(offset of the first malformed line) - 1"""
    out, at, n = [], 0, 0
    while at < len(sam):
        nl = sam.find(b"\n", at)
        if nl < 0:
            return -at - 1, 0
        try:
            out.append(encode_record(sam[at:nl], names))
        except Malformed:
            return -at - 1, 0
        n += 1
        at = nl + 1
    return b"".join(out), n


def encode_header(text, contigs):
    """contigs: (name, length) in order"""
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(contigs))
    for name, length in contigs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return out


def cuts(records):
    """the payload sizes of the BGZF blocks over a list of records: as many whole records as fit BLOCK bytes; a record that alone is
    larger is cut into blocks of BLOCK bytes"""
    out, cur = [], 0
    for r in records:
        if cur and cur + len(r) > BLOCK:
            out.append(cur)
            cur = 0
        if len(r) > BLOCK:
            assert cur == 0
            left = len(r)
            while left > BLOCK:
                out.append(BLOCK)
                left -= BLOCK
            out.append(left)
            continue
        cur += len(r)
    if cur:
        out.append(cur)
    return out


# ---- the decoder ----
def decode_header(data):
    """-> (header text, [(name, length)], offset of the first record)"""
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", data, 4)
    text = data[8:8 + l_text]
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, at)
    at += 4
    contigs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, at)
        name = data[at + 4:at + 4 + l_name]
        assert name.endswith(b"\0") and b"\0" not in name[:-1]
        length, = struct.unpack_from("<i", data, at + 4 + l_name)
        contigs.append((name[:-1], length))
        at += 8 + l_name
    return text, contigs, at


def split_records(data, at=0):
    """the records of data[at:] by their block_size chain"""
    out = []
    while at < len(data):
        size, = struct.unpack_from("<i", data, at)
        assert size >= 32 and at + 4 + size <= len(data), (at, size)
        out.append(data[at:at + 4 + size])
        at += 4 + size
    return out


def _float_text(bits):
    return b"f32:%08x" % bits   # (floats are compared as float32: see normalise())


def decode_record(rec, names):
    """one record as a SAM line (no newline); 'f' values are printed as their float32 bits"""
    size, refid, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, next_refid, next_pos, tlen = struct.unpack_from("<iiiBBHHHiiii", rec, 0)
    assert size == len(rec) - 4
    at = 36
    qname = rec[at:at + l_name]
    assert qname.endswith(b"\0")
    at += l_name
    cigar = b""
    ref_len = 0
    for _ in range(n_cigar):
        w, = struct.unpack_from("<I", rec, at)
        cigar += b"%d%s" % (w >> 4, CIGAR_OPS[w & 15].encode())
        if CIGAR_OPS[w & 15] in "MDN=X":
            ref_len += w >> 4
        at += 4
    assert bin_ == reg2bin(pos, pos + (ref_len if ref_len else 1)) & 0xffff
    packed = rec[at:at + (l_seq + 1) // 2]
    at += (l_seq + 1) // 2
    seq = "".join(SEQ_CODES[b >> 4] + SEQ_CODES[b & 15] for b in packed)[:l_seq].encode()
    if l_seq & 1:
        assert packed[-1] & 15 == 0
    qual = rec[at:at + l_seq]
    at += l_seq
    qual = b"*" if (l_seq == 0 or all(q == 0xff for q in qual)) else bytes((q + 33) & 0xff for q in qual)
    tags = []
    while at < len(rec):
        name, kind = rec[at:at + 2], chr(rec[at + 2])
        at += 3
        if kind == "A":
            tags.append(name + b":A:" + rec[at:at + 1])
            at += 1
        elif kind in "cCsSiI":
            fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[kind]
            v, = struct.unpack_from(fmt, rec, at)
            tags.append(name + b":i:%d" % v)
            at += struct.calcsize(fmt)
        elif kind == "f":
            tags.append(name + b":f:" + _float_text(struct.unpack_from("<I", rec, at)[0]))
            at += 4
        elif kind in "ZH":
            end = rec.index(b"\0", at)
            tags.append(name + b":" + kind.encode() + b":" + rec[at:end])
            at = end + 1
        elif kind == "B":
            sub = chr(rec[at])
            count, = struct.unpack_from("<i", rec, at + 1)
            at += 5
            vals = []
            for _ in range(count):
                if sub == "f":
                    vals.append(_float_text(struct.unpack_from("<I", rec, at)[0]))
                    at += 4
                else:
                    fmt = _ARRAY[sub][0]
                    vals.append(b"%d" % struct.unpack_from(fmt, rec, at)[0])
                    at += struct.calcsize(fmt)
            tags.append(name + b":B:" + b",".join([sub.encode()] + vals))
        else:
            raise AssertionError("tag type %r" % kind)
    assert at == len(rec)

    def ref(i):
        return b"*" if i < 0 else names[i]
    rnext = b"*" if next_refid < 0 else b"=" if next_refid == refid else names[next_refid]
    fields = [qname[:-1], b"%d" % flag, ref(refid), b"%d" % (pos + 1), b"%d" % mapq, cigar or b"*", rnext, b"%d" % (next_pos + 1), b"%d" % tlen,
              seq or b"*", qual] + tags
    return b"\t".join(fields)


def normalise(line):
    """a SAM line as decode_record prints it: floats as float32 bits, upper-case bases, RNEXT '=' where it names RNAME"""
    f = line.split(b"\t")
    if f[6] == f[2] and f[2] != b"*":
        f[6] = b"="
    if f[6] == b"=" and f[2] == b"*":
        f[6] = b"*"
    if f[9] != b"*":
        f[9] = bytes(c if chr(c) in SEQ_CODES else ord("N") for c in f[9].upper())
    for k in range(11, len(f)):
        if f[k][3:4] == b"f":
            f[k] = f[k][:5] + _float_text(float32_bits(f[k][5:]))
        elif f[k][3:4] == b"i":
            f[k] = f[k][:5] + b"%d" % int(f[k][5:])
        elif f[k][3:4] == b"B" and f[k][5:6] == b"f":
            p = f[k][5:].split(b",")
            f[k] = f[k][:5] + b",".join([p[0]] + [_float_text(float32_bits(x)) for x in p[1:]])
    return b"\t".join(f)


def bgzf_blocks(data):
    """(block, payload) of a BGZF stream; every block is checked as a gzip member with the 'BC' field"""
    import zlib
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 10:at + 16] == b"\x06\x00BC\x02\x00", at
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        blk = data[at:at + bsize]
        assert len(blk) == bsize
        payload = zlib.decompress(blk[18:-8], -15)
        crc, isize = struct.unpack_from("<II", blk, bsize - 8)
        assert isize == len(payload) and crc == zlib.crc32(payload)
        out.append((blk, payload))
        at += bsize
    return out
