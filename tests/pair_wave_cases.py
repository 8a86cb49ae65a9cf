"""Pairs for pair_wave_kernel (mpibwa_amd/csrc/pair_wave_kernel.hip) and what the reference alone makes of them, for the stage test
(tests/test_gpu_pair_wave_stage.py), the end-to-end test (tests/test_gpu_pair_wave_e2e.py) and their CPU companion
(tests/test_pair_wave_cases.py).

The recipe.  Genome: simulate.make_genome(400_000, 3, seed=GENOME_SEED, repeat_frac=0.2), then two planted families with rng
default_rng(FAMILY_SEED): a 700 bp unit in 55 copies diverged 2 % and a 350 bp unit in 48 copies diverged 3 % (substitutions; every
second copy reverse-complemented; the copies never overlap an N run's contig end).  Reads: simulate.simulate_reads(seqs, 1500, 150,
paired=True, seed=READ_SEED, frac_random=0.0) plus 400 pairs whose fragment starts inside or next to a planted copy (so that an end
carries dozens of regions and its mate sits in unique sequence).  "Damaged": mate 2 of every second pair gets substitutions at a rate
drawn uniformly from 6-20 % — the reads whose mate has few or no seeds, the ordinary case of mate rescue.

The reference's side: mem_align1_core regions per read and the chunk's mem_pestat (tests/test_host_pair.py::_batch), then its own
mem_sam_pe per pair with id = the pair's number.  A pair is ELIGIBLE, from the reference alone, when mem_sam_pe attempted a rescue
alignment or an end has more than eight regions; both lists hold at most 64 regions before and after the call; each read's text is one
line without XA:Z / SA:Z / pa:f; and both flags carry 0x2."""
import ctypes as C

import numpy as np

from c2a_cases import _alnreg_v, _ref_handle, _regs_copy
from oracle import pyoracle as po

GENOME_SEED = 23
FAMILY_SEED = 6
READ_SEED = 61
COPY_SEED = 62
DAMAGE_SEED = 63
FAMILIES = ((700, 55, 0.02), (350, 48, 0.03))
N_PLAIN, N_AT_COPIES = 1500, 400
_COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


def build_genome():
    """-> names, seqs, copies [(contig, position, length)]"""
    from mpibwa_amd import simulate
    names, seqs = simulate.make_genome(400_000, 3, seed=GENOME_SEED, repeat_frac=0.2)
    rng = np.random.default_rng(FAMILY_SEED)
    copies = []
    for unit_len, n_copies, div in FAMILIES:
        unit = rng.integers(0, 4, unit_len).astype(np.uint8)
        for k in range(n_copies):
            c = int(rng.integers(0, len(seqs)))
            p = int(rng.integers(2000, len(seqs[c]) - unit_len - 2000))
            cp = unit.copy()
            m = rng.random(unit_len) < div
            cp[m] = (cp[m] + rng.integers(1, 4, int(m.sum())).astype(np.uint8)) & 3
            if k % 2:
                cp = _COMP[cp[::-1]]
            seqs[c][p:p + unit_len] = cp
            copies.append((c, p, unit_len))
    return names, seqs, copies


def make_reads(seqs, copies, damaged):
    """-> [(name, mate 1, mate 2)] code arrays"""
    from mpibwa_amd import simulate
    reads = simulate.simulate_reads(seqs, N_PLAIN, 150, paired=True, seed=READ_SEED, frac_random=0.0)
    rng = np.random.default_rng(COPY_SEED)
    for k in range(N_AT_COPIES):
        c, p, ln = copies[int(rng.integers(0, len(copies)))]
        fl = int(max(rng.normal(400.0, 50.0), 170))
        start = p + int(rng.integers(-fl + 60, ln - 60))
        start = max(0, min(start, len(seqs[c]) - fl - 1))
        frag = seqs[c][start:start + fl].copy()
        n_mask = frag > 3
        frag[n_mask] = rng.integers(0, 4, int(n_mask.sum())).astype(np.uint8)
        if rng.random() < 0.5:
            frag = _COMP[frag[::-1]]
        frag = simulate._mutate(frag, rng, 0.01, 0.001)
        reads.append(("c%d" % k, frag[:150].copy(), _COMP[frag[::-1]][:150].copy()))
    if damaged:
        rng = np.random.default_rng(DAMAGE_SEED)
        out = []
        for k, (name, a, b) in enumerate(reads):
            if k % 2:
                b = b.copy()
                m = (rng.random(len(b)) < rng.uniform(0.06, 0.20)) & (b < 4)
                b[m] = (b[m] + rng.integers(1, 4, int(m.sum())).astype(np.uint8)) & 3
            out.append((name, a, b))
        reads = out
    return reads


def build_index(directory):
    """the case genome on disk with its index -> dict(prefix, names, seqs, copies)"""
    from mpibwa_amd import api, simulate
    names, seqs, copies = build_genome()
    fa = str(directory / "pw.fa")
    simulate.write_fasta(fa, names, seqs)
    api.build_index(fa, fa)
    return {"prefix": fa, "names": names, "seqs": seqs, "copies": copies}


def quality(n, k):
    return bytes(33 + (7 * i + k) % 40 for i in range(n))


class Pair:
    """one pair as the reference sees it"""
    __slots__ = ("name", "reads", "before", "after", "n_rescue", "text")

    @property
    def n_before(self):
        return (len(self.before[0]), len(self.before[1]))

    @property
    def lines(self):
        return [t.splitlines() for t in self.text]

    @property
    def plain(self):
        """one line per read without XA / SA / pa"""
        return all(len(ln) == 1 and b"\tXA:Z:" not in ln[0] and b"\tSA:Z:" not in ln[0] and b"\tpa:f:" not in ln[0] for ln in self.lines)

    @property
    def eligible(self):
        if not (self.n_rescue > 0 or max(self.n_before) > 8):
            return False
        if max(self.n_before) > 64 or max(len(self.after[0]), len(self.after[1])) > 64 or not self.plain:
            return False
        return all(int(ln[0].split(b"\t")[1]) & 0x2 for ln in self.lines)


def reference_side(ref, opt, reads):
    """reads: [(name, ACGT bytes, ACGT bytes)] -> (list of Pair, the chunk's mem_pestat)"""
    from mpibwa_amd import abi, api
    from test_host_pair import _batch
    R = _ref_handle()
    R.mem_sam_pe.restype = C.c_int
    R.mem_sam_pe.argtypes = [C.POINTER(abi.mem_opt_t), C.POINTER(abi.bntseq_t), C.POINTER(C.c_uint8), C.POINTER(abi.mem_pestat_t), C.c_uint64,
                             C.POINTER(abi.bseq1_t), C.POINTER(_alnreg_v)]
    regs, seqs, pes = _batch(ref, R, opt, reads)
    out = []
    for p, (name, _, _) in enumerate(reads):
        P = Pair()
        P.name = name.encode() if isinstance(name, str) else name
        nm = C.create_string_buffer(P.name)
        P.reads = [np.frombuffer(seqs[2 * p + k].raw[:-1], dtype=np.uint8).copy() for k in range(2)]
        qual = [C.create_string_buffer(quality(len(P.reads[k]), p)) for k in range(2)]
        P.before = [_regs_copy(regs[2 * p + k]) for k in range(2)]
        s = (abi.bseq1_t * 2)()
        for k in range(2):
            s[k].l_seq = len(P.reads[k])
            s[k].name = C.addressof(nm)
            s[k].seq = C.addressof(seqs[2 * p + k])
            s[k].qual = C.addressof(qual[k])
        a = (_alnreg_v * 2)(regs[2 * p], regs[2 * p + 1])
        P.n_rescue = R.mem_sam_pe(opt, ref.bns, ref.pac, pes, p, s, a)
        P.after = [_regs_copy(a[k]) for k in range(2)]
        P.text = []
        for k in range(2):
            P.text.append(C.string_at(s[k].sam))
            api.libc.free(C.c_void_p(s[k].sam))
            api.libc.free(C.c_void_p(a[k].a))
        out.append(P)
    return out, pes


def census(pairs):
    """the counts the CPU test puts floors under"""
    el = [P for P in pairs if P.eligible]
    return {
        "pairs": len(pairs),
        "eligible": len(el),
        "eligible_33_64": sum(1 for P in el if max(P.n_before) > 32),
        "eligible_from_no_region": sum(1 for P in el if min(P.n_before) == 0),
        "xa_or_extra_lines": sum(1 for P in pairs if not P.plain),
    }
