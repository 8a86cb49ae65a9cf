"""mi355x_bgzf_compress_dev (csrc/bgzf_kernel.hip, csrc/bgzf_stage.hip): BGZF blocks made by the deflate kernel.

Every case: each block is a gzip member with the 'BC' field, BSIZE, the CRC32 and ISIZE of its payload, and a raw deflate stream that
zlib inflates; the payloads are the text, cut where the host path cuts it; a second call gives the same bytes.  The cases are the ends
of the encoder: texts shorter than a hash's four bytes, blocks of one byte value, a block without any match, candidates just inside
and just outside the window of 32 768, a code that wants to be deeper than 15 bits, text that does not compress (stored blocks).

Compression is held against zlib on the same cuts, run inside the test: the device's total is below zlib's Z_HUFFMAN_ONLY total
(matches are found and used) and below its Z_FIXED level-1 total (the dynamic codes earn their header), and within 5 % of the ratio
to zlib level 1 that was measured once on an MI355X (the output is deterministic: the slack is for a later change of the test text)."""
import ctypes as C
import gzip
import os
import struct
import threading
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EX = os.path.join(HERE, "golden", "mpibwa_examples")
BLOCK = 0xff00
Z_HUFFMAN_ONLY, Z_FIXED = 2, 4

# device bytes / zlib level-1 bytes on the same cuts, measured on an MI355X
MEASURED_VS_LEVEL1 = {"ordinary": 0.9500, "real": 0.9984}


@pytest.fixture(scope="module")
def lib(built):
    from mpibwa_amd import api
    return api.load_library()


def _bgzf_blocks(data):
    """[(block bytes, payload)] of a BGZF stream, every header field checked (SAM spec 4.1)"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 10:at + 12] == b"\x06\x00" and data[at + 12:at + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        blk = data[at:at + bsize]
        assert len(blk) == bsize
        payload = zlib.decompress(blk[18:-8], -15)
        crc, isize = struct.unpack("<II", blk[-8:])
        assert crc == zlib.crc32(payload) and isize == len(payload) and bsize <= 65536
        out.append((blk, payload))
        at += bsize
    assert at == len(data)
    return out


def _dev(lib, t, cap=None):
    cap = lib.mi355x_bgzf_bound(len(t)) if cap is None else cap
    out = C.create_string_buffer(max(cap, 1))
    n = lib.mi355x_bgzf_compress_dev(t, len(t), out, cap)
    return out.raw[:n]


def _host_lengths(lib, t):
    cap = lib.mi355x_bgzf_bound(len(t))
    out = C.create_string_buffer(max(cap, 1))
    n = lib.mi355x_bgzf_compress(t, len(t), 1, out, cap)
    return [len(p) for _, p in _bgzf_blocks(out.raw[:n])]


def _counts(lib):
    c = (C.c_uint64 * 4)()
    lib.mi355x_bgzf_dev_counts(c)
    return list(c)


def _check(lib, t):
    """the checks of every case; returns the blocks"""
    data = _dev(lib, t)
    blocks = _bgzf_blocks(data)
    assert b"".join(p for _, p in blocks) == t
    if t:
        assert gzip.decompress(data) == t
    assert [len(p) for _, p in blocks] == _host_lengths(lib, t)
    assert _dev(lib, t) == data
    return blocks


def _stored(blk):
    return blk[18] & 7 == 1   # BFINAL, BTYPE 00


def _max_distance(blk):
    """the largest match distance in a block's deflate stream (0: no match), by reading the stream: one dynamic block (RFC 1951 3.2.7)"""
    data, pos = blk[18:-8], 0

    def bits(n):
        nonlocal pos
        v = 0
        for k in range(n):
            v |= ((data[(pos + k) >> 3] >> ((pos + k) & 7)) & 1) << k
        pos += n
        return v

    def table(lens):
        code, out = 0, {}
        for ln in range(1, 16):
            for sym, l in enumerate(lens):
                if l == ln:
                    out[(ln, code)] = sym
                    code += 1
            code <<= 1
        return out

    def sym(tab):
        code = 0
        for ln in range(1, 16):
            code = code << 1 | bits(1)
            if (ln, code) in tab:
                return tab[(ln, code)]
        raise AssertionError("no such code")
    assert bits(3) == 5                                   # last block, dynamic codes
    hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
    cl = [0] * 19
    for k in range(hclen):
        cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[k]] = bits(3)
    cl, lens = table(cl), []
    while len(lens) < hlit + hdist:
        c = sym(cl)
        if c < 16:
            lens.append(c)
        elif c == 16:
            lens += [lens[-1]] * (3 + bits(2))
        else:
            lens += [0] * (3 + bits(3) if c == 17 else 11 + bits(7))
    ll, dd, far = table(lens[:hlit]), table(lens[hlit:]), 0
    while True:
        c = sym(ll)
        if c == 256:
            return far
        if c > 256:
            if 264 < c < 285:
                bits((c - 261) >> 2)
            d = sym(dd)
            far = max(far, d + 1 if d < 4 else ((2 + (d & 1)) << ((d >> 1) - 1)) + 1 + bits((d >> 1) - 1))


@pytest.fixture(scope="module")
def ordinary():
    rng = np.random.default_rng(4)

    def record(n):
        return b"r%d\t99\tchr1\t%d\t60\t%dM\t=\t%d\t400\t" % (n, n * 7, 150, n * 7 + 250) + bytes(rng.choice(list(b"ACGT"), 150).tolist()) + b"\t" + \
            bytes((rng.integers(2, 42, 150) + 33).astype(np.uint8).tolist()) + b"\tNM:i:0\tMD:Z:150\tAS:i:150\tXS:i:0\n"
    recs = [record(n) for n in range(4000)]
    return recs, b"".join(recs)   # 1.5 MB of ordinary records (random bases and qualities), as the host test builds them


@pytest.fixture(scope="module")
def real():
    """the example reads laid out as SAM-like records with their real qualities, about 3 MB"""
    rng = np.random.default_rng(9)
    out = []
    with gzip.open(os.path.join(EX, "HCC1187C_R1_10K.fastq.gz"), "rb") as g:
        lines = g.read().split(b"\n")
    for k in range(0, len(lines) - 3, 4):
        name, seq, qual = lines[k][1:].split()[0], lines[k + 1], lines[k + 3]
        pos = int(rng.integers(1, 50_000_000))
        out.append(b"%s\t%d\tchr%d\t%d\t60\t%dM\t=\t%d\t%d\t%s\t%s\tNM:i:%d\tMD:Z:%d\tAS:i:%d\tXS:i:%d\n" % (
            name, 99 if k % 8 else 147, 1 + k % 22, pos, len(seq), pos + 250, 350, seq, qual, k % 3, len(seq), len(seq) - k % 7, k % 40))
    t = b"".join(out)
    assert 2_500_000 < len(t) < 4_000_000
    return t


def test_short_texts_and_one_record(lib, ordinary):
    c0 = _counts(lib)
    assert _dev(lib, b"") == b"" and lib.mi355x_bgzf_compress_dev(b"", 0, None, 0) == 0
    assert _counts(lib) == c0
    for t in (b"A", b"AB", b"ABC", b"ABCD", b"AAAAA", ordinary[0][1]):
        assert len(_check(lib, t)) == 1
    c1 = _counts(lib)
    assert c1[0] - c0[0] == 12 and c1[2] - c0[2] == 2 * (1 + 2 + 3 + 4 + 5 + len(ordinary[0][1]))   # two calls per text


@pytest.mark.parametrize("which", ["ordinary", "real"])
def test_sam_text_compresses_with_matches_and_dynamic_codes(lib, ordinary, real, which):
    t = ordinary[1] if which == "ordinary" else real
    blocks = _check(lib, t)
    assert all(p.endswith(b"\n") for _, p in blocks) and all(len(p) > 60000 for _, p in blocks[:-1])
    assert not any(_stored(b) for b, _ in blocks)

    def z(p, level, strategy):
        o = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        return len(o.compress(p) + o.flush())
    dev = sum(len(b) - 26 for b, _ in blocks)
    huff = sum(z(p, 1, Z_HUFFMAN_ONLY) for _, p in blocks)
    fixed = sum(z(p, 1, Z_FIXED) for _, p in blocks)
    lvl1 = sum(z(p, 1, zlib.Z_DEFAULT_STRATEGY) for _, p in blocks)
    lvl3 = sum(z(p, 3, zlib.Z_DEFAULT_STRATEGY) for _, p in blocks)
    print("\n[bgzf %s] text %d  device %d (%.4f)  zlib huffman-only %d (%.4f)  fixed level 1 %d (%.4f)  level 1 %d (%.4f)  level 3 %d (%.4f)  device / level 1 = %.4f" % (
        which, len(t), dev, dev / len(t), huff, huff / len(t), fixed, fixed / len(t), lvl1, lvl1 / len(t), lvl3, lvl3 / len(t), dev / lvl1))
    assert dev < huff
    assert dev < fixed
    assert dev <= MEASURED_VS_LEVEL1[which] * 1.05 * lvl1


def test_a_record_longer_than_a_block_and_runs_of_one_byte(lib, ordinary):
    text = ordinary[1]
    long_line = b"x\t4\t*\t0\t0\t*\t*\t0\t0\t" + b"A" * 200000 + b"\t" + b"I" * 200000 + b"\n"
    blocks = _check(lib, text[:70000] + long_line + text[70000:140000])
    runs = [b for b, p in blocks if len(p) == BLOCK and len(set(p)) == 1]
    assert len(runs) >= 4                                  # blocks that are one byte value: one literal, then matches of 258
    assert all(len(b) < 400 and not _stored(b) for b in runs)


def test_block_of_exactly_the_limit_and_one_more(lib):
    rng = np.random.default_rng(1)
    base = bytes(rng.choice(list(b"ACGTN\t"), BLOCK + 1).tolist())
    assert [len(p) for _, p in _check(lib, base[:BLOCK])] == [BLOCK]
    assert [len(p) for _, p in _check(lib, base)] == [BLOCK, 1]


def test_text_that_does_not_compress_is_stored(lib):
    t = bytes(np.random.default_rng(2).integers(0, 256, 300000).astype(np.uint8).tolist())
    c0 = _counts(lib)
    blocks = _check(lib, t)
    c1 = _counts(lib)
    assert all(_stored(b) and len(b) == len(p) + 31 for b, p in blocks)
    assert c1[0] - c0[0] == 2 * len(blocks) and c1[1] - c0[1] == 2 * len(blocks)   # (_check calls twice)
    assert c1[2] - c0[2] == 2 * len(t) and c1[3] - c0[3] == 2 * sum(len(b) for b, _ in blocks)


def test_a_candidate_beyond_the_window_is_refused(lib):
    """A block of 65 280 bytes whose second half repeats its first half: at distance 32 640 the repeat is a run of matches, at 32 769 every
    candidate lies one byte too far and the block inflates correctly only because the encoder refused them.  The halves are 3 000
    random bytes and a filler of one byte value, so that the random bytes' places in the hash table survive the bytes between."""
    rng = np.random.default_rng(3)
    size = {}
    for dist in (32640, 32769):
        half = bytes(rng.integers(0, 256, 3000).astype(np.uint8).tolist()) + b"\0" * (dist - 3000)
        t = (half + half)[:BLOCK]
        assert len(t) == BLOCK and t[dist:dist + 3000] == t[:3000]
        (blk, payload), = _check(lib, t)
        assert payload == t and not _stored(blk)
        size[dist] = len(blk)
        if dist == 32640:
            assert _max_distance(blk) == 32640      # the repeat is coded as matches at that distance
        else:
            assert 0 < _max_distance(blk) <= 32768
    assert size[32640] < 4000 and size[32769] > size[32640] + 2500   # the refused repeat is literals again


def test_every_byte_value_once_has_no_match_and_no_distance_code(lib):
    t = bytes(np.random.default_rng(5).permutation(256).astype(np.uint8).tolist())
    (blk, _), = _check(lib, t)
    _check(lib, bytes(range(256)) * 3)         # and with matches again, at distance 256
    # long enough for the dynamic codes to pay (the 256 bytes above are smaller stored): 1 500 bytes over 64 values in which no four
    # bytes come twice, so no position has a match and the distance alphabet is empty
    for seed in range(100):
        t = bytes((np.random.default_rng(seed).integers(0, 64, 1500) + 48).astype(np.uint8).tolist())
        if len({t[k:k + 4] for k in range(len(t) - 3)}) == len(t) - 3:
            break
    assert len({t[k:k + 4] for k in range(len(t) - 3)}) == len(t) - 3
    (blk, _), = _check(lib, t)
    assert not _stored(blk) and len(blk) < 1400 and _max_distance(blk) == 0


def test_frequencies_that_want_a_code_deeper_than_15_bits(lib):
    rng = np.random.default_rng(6)
    fib, sym = [1, 1], []
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    for k, f in enumerate(fib):
        sym += [65 + k] * f
    assert len(sym) > BLOCK                    # 121 392 symbols: two blocks, the first with the whole spread of frequencies
    t = bytes(rng.permutation(np.array(sym, dtype=np.uint8)).tolist())
    blocks = _check(lib, t)
    assert not any(_stored(b) for b, _ in blocks)


def test_blocks_are_independent_and_a_small_buffer_is_refused(lib, ordinary):
    t = ordinary[1][:300000]
    a = _bgzf_blocks(_dev(lib, t))
    b = _bgzf_blocks(_dev(lib, t + b"extra\trecord\twithout\tan\tend"))
    assert len(a) >= 4 and [x for x, _ in a[:-1]] == [x for x, _ in b[:len(a) - 1]]
    assert lib.mi355x_bgzf_compress_dev(t, len(t), C.create_string_buffer(65536), 65536) == 0   # room for one block only


def test_callers_side_by_side_and_beside_the_aligner(lib, ordinary, real, genome, reads_pe):
    from mpibwa_amd import abi, api, simulate
    texts = [ordinary[1], real[:1_000_000], ordinary[1][:200_000], real[1_000_000:1_700_000], b"A" * 100_000, ordinary[1][5:333_333],
             bytes(np.random.default_rng(8).integers(0, 256, 150_000).astype(np.uint8).tolist()), real[2_000_000:2_000_777]]
    want = [_dev(lib, t) for t in texts]
    lib.mi355x_finalize()                      # no context has buffers: the first round below, eight calls started together, makes all eight
    eng = api.Engine(genome["prefix"], device=0)
    opt, ra = eng.opt(flag=abi.MEM_F_PE), simulate.reads_to_ascii(reads_pe)
    sam = eng.process(opt, ra)
    for _ in range(2):
        assert eng.process(opt, ra) == sam
    rounds, gate, bad, marks, stop = 16, threading.Barrier(8), [], [], threading.Event()

    def caller(k):
        for r in range(rounds):
            i = gate.wait(timeout=600)
            if r == 1 and i == 0:
                marks.append(int(lib.mi355x_buffer_growths()))   # every context has its buffers after the first round
            if _dev(lib, texts[k]) != want[k]:
                bad.append((k, r))

    def aligner():
        while not stop.is_set():
            if eng.process(opt, ra) != sam:
                bad.append("sam")
    th = [threading.Thread(target=caller, args=(k,)) for k in range(8)]
    al = threading.Thread(target=aligner)
    al.start()
    for x in th:
        x.start()
    for x in th:
        x.join()
    stop.set()
    al.join()
    assert not bad
    assert int(lib.mi355x_buffer_growths()) == marks[0]
    lib.mi355x_finalize()
    assert _dev(lib, texts[2]) == want[2]      # the contexts come back after mi355x_finalize has given their buffers away
