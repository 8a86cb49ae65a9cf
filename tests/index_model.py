"""A plain model of the bwa-format FM-index, written from the format description alone (src/bwt.c:385-462 and src/bwt.h:72-73 as
restated at the top of csrc/index.cpp): the known answer of both index builders on the genomes of tests/index_cases.py.  numpy only; it
shares no code with csrc/index.cpp or csrc/index_gpu.hip.  tests/test_index_cases.py ties it to the reference: it reproduces the
reference's own hg19.small .bwt and .sa byte for byte.

The text is the forward strand followed by its reverse complement, N = 2 l_pac symbols, and a sentinel smaller than every base.
Row r of the index is the r-th smallest suffix; row 0 is the sentinel's; `primary` is the row of the whole text."""
import numpy as np

SA_INTV = 32
OCC_INTV = 128


def pack_pac(codes):
    """bases 0..3 -> 2 bits per base, first base in a byte's top bits; l_pac // 4 + 1 bytes (what mi355x_index_build_gpu reads)"""
    codes = np.asarray(codes, np.uint8)
    n = len(codes)
    pad = np.zeros((n // 4 + 1) * 4, np.uint8)
    pad[:n] = codes
    q = pad.reshape(-1, 4)
    return (q[:, 0] << 6 | q[:, 1] << 4 | q[:, 2] << 2 | q[:, 3]).astype(np.uint8)


def unpack_pac(pac, l_pac):
    pac = np.asarray(pac, np.uint8)
    i = np.arange(l_pac)
    return ((pac[i >> 2] >> ((3 - (i & 3)) * 2)) & 3).astype(np.uint8)


def read_pac_file(prefix):
    """-> the bases of <prefix>.pac: its last byte is l_pac % 4, before it a zero byte when that is 0 (src/bntseq.c:317-325)"""
    raw = np.fromfile(prefix + ".pac", dtype=np.uint8)
    l_pac = (len(raw) - 2) * 4 + int(raw[-1])
    assert l_pac == int(open(prefix + ".ann").readline().split()[0])
    return unpack_pac(raw, l_pac)


def text_of(fwd_codes):
    fwd = np.asarray(fwd_codes, np.uint8)
    return np.concatenate([fwd, (3 - fwd)[::-1]]).astype(np.uint8)


def suffix_array_sorted(codes):
    """the definition itself: the suffixes of codes + sentinel, compared as sequences"""
    s = [int(c) + 1 for c in codes] + [0]
    return np.array(sorted(range(len(s)), key=lambda i: s[i:]), dtype=np.int64)


def suffix_array(codes, with_rounds=False):
    """prefix doubling: after the round with step h the ranks order the suffixes by their first 2 h symbols"""
    n = len(codes) + 1
    rank = np.zeros(n, np.int64)
    rank[:-1] = np.asarray(codes, np.int64) + 1
    h, rounds = 1, 0
    while True:
        second = np.full(n, -1, np.int64)
        second[:n - h] = rank[h:]
        order = np.lexsort((second, rank))
        r, s = rank[order], second[order]
        new = np.zeros(n, np.int64)
        new[1:] = np.cumsum((r[1:] != r[:-1]) | (s[1:] != s[:-1]))
        rank = np.empty(n, np.int64)
        rank[order] = new
        rounds += 1
        if new[-1] == n - 1:
            break
        h <<= 1
    sa = order.astype(np.int64)
    if n <= 65:
        assert (sa == suffix_array_sorted(codes)).all()
    return (sa, rounds) if with_rounds else sa


def index_files(fwd_codes, with_info=False):
    """-> (bytes of .bwt, bytes of .sa, the whole suffix array [N + 1 rows])"""
    T = text_of(fwd_codes)
    N = len(T)
    sa, rounds = suffix_array(T, with_rounds=True)
    primary = int(np.flatnonzero(sa == 0)[0])
    B = T[sa[sa != 0] - 1]                                   # the symbol before each suffix, the row of the whole text left out
    assert len(B) == N
    L2 = np.concatenate([[0], np.cumsum(np.bincount(T, minlength=4))]).astype(np.uint64)
    head = np.concatenate([[np.uint64(primary)], L2[1:]]).astype("<u8")
    # running counts before every 128th symbol, and the closing totals
    onehot = (B[:, None] == np.arange(4)[None, :]).astype(np.uint64)
    run = np.concatenate([np.zeros((1, 4), np.uint64), np.cumsum(onehot, axis=0, dtype=np.uint64)])
    n_blk = (N + OCC_INTV - 1) // OCC_INTV
    n_words = (N + 15) // 16
    pad = np.zeros(n_words * 16, np.uint32)
    pad[:N] = B
    words = np.zeros(n_words, np.uint32)
    for k in range(16):
        words |= pad[k::16] << np.uint32(2 * (15 - k))
    parts = [head.tobytes()]
    for b in range(n_blk):
        parts.append(run[b * OCC_INTV].astype("<u8").tobytes())
        parts.append(words[b * 8:(b + 1) * 8].astype("<u4").tobytes())
    parts.append(run[N].astype("<u8").tobytes())
    bwt = b"".join(parts)
    n_sa = (N + SA_INTV) // SA_INTV
    sa_file = np.concatenate([head, np.array([SA_INTV, N], "<u8"), sa[SA_INTV::SA_INTV][:n_sa - 1].astype("<u8")]).tobytes()
    assert len(sa[SA_INTV::SA_INTV]) == n_sa - 1
    if with_info:
        return bwt, sa_file, sa, dict(primary=primary, rounds=rounds, N=N, L2=[int(v) for v in L2])
    return bwt, sa_file, sa
