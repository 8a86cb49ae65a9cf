"""What the reference alone says about XA tags on the pairs of tests/pair_wave_cases.py, for the stage test of the XA listing
(tests/test_gpu_xa_stage.py), the end-to-end test (tests/test_gpu_xa_e2e.py) and their CPU companion (tests/test_xa_cases.py).

A pair is XA-ONLY when its records differ from plain ones by an XA tag alone: one line per read, XA:Z: on at least one of the two, no
SA:Z: / pa:f:, both flags with 0x2, and both region lists within 64 before and after mem_sam_pe.  These are the pairs pair_wave_kernel
decides with status PW_DECIDED_XA."""


def xa_tag(line):
    """the value of a record's XA tag (b"" without one)"""
    for f in line.rstrip(b"\n").split(b"\t")[11:]:
        if f.startswith(b"XA:Z:"):
            return f[5:]
    return b""


def xa_lines(P):
    """P: pair_wave_cases.Pair -> one line per read, XA:Z: on at least one, no SA:Z: / pa:f:"""
    ln = P.lines
    if not all(len(x) == 1 and b"\tSA:Z:" not in x[0] and b"\tpa:f:" not in x[0] for x in ln):
        return False
    return any(b"\tXA:Z:" in x[0] for x in ln)


def xa_only(P):
    ln = P.lines
    if not xa_lines(P):
        return False
    if max(P.n_before) > 64 or max(len(P.after[0]), len(P.after[1])) > 64:
        return False
    return all(int(x[0].split(b"\t")[1]) & 0x2 for x in ln)


def census(pairs):
    """the counts tests/test_xa_cases.py puts floors under"""
    xo = [P for P in pairs if xa_only(P)]
    tags = [t for P in xo for t in (xa_tag(x[0]) for x in P.lines) if t]
    by_entries = {}
    for t in tags:
        by_entries[t.count(b";")] = by_entries.get(t.count(b";"), 0) + 1
    return {
        "pairs": len(pairs),
        "xa_only": len(xo),
        "with_rescue": sum(1 for P in xo if P.n_rescue > 0),
        "over_8_regions": sum(1 for P in xo if max(P.n_before) > 8),
        "tags_by_entries": dict(sorted(by_entries.items())),
        "longest_tag": max((len(b"XA:Z:") + len(t) for t in tags), default=0),
        "most_cigar_ops": max((sum(ch.isalpha() for ch in e.split(b",")[2].decode()) for t in tags for e in t.split(b";") if e), default=0),
    }
