"""One text over three pieces of the device BAM stage (csrc/device.h: BAM_DEV_TEXT = 24 MB), for tests/test_gpu_bam.py:

    python tests/bam_three_pieces.py TEXT_FILE CONTIGS_JSON

The text is repeated until it spans three pieces; mi355x_bam_compress_dev's payload, mi355x_sam_to_bam_dev's records and
mi355x_sam_to_bam's records must be the same bytes.  The case holds a few hundred MB of buffers, so it runs in a process of its own:
the suite's process keeps its memory state (tests/test_gpu_soak.py watches the resident set)."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import bam_model as bm  # noqa: E402

PIECE = 24 << 20


def main():
    from mpibwa_amd import abi, api
    text = open(sys.argv[1], "rb").read()
    contigs = [(n.encode(), l) for n, l in json.load(open(sys.argv[2]))]
    anns = (abi.bntann1_t * len(contigs))()
    for i, (n, l) in enumerate(contigs):
        anns[i].name, anns[i].anno, anns[i].len = n, b"", l
    bns = abi.bntseq_t()
    bns.n_seqs, bns.anns = len(contigs), anns
    lib = api.load_library()
    big = text * ((2 * PIECE) // len(text) + 2)
    assert 2 * PIECE < len(big) < 3 * PIECE
    cap = lib.mi355x_bgzf_bound(lib.mi355x_bam_bound(len(big)))
    out = C.create_string_buffer(cap)
    size = lib.mi355x_bam_compress_dev(big, len(big), C.byref(bns), out, cap)
    assert size > 0, size
    payload = b"".join(p for _, p in bm.bgzf_blocks(out.raw[:size]))
    hcap = lib.mi355x_bam_bound(len(big))
    hout = C.create_string_buffer(hcap)
    hsize = lib.mi355x_sam_to_bam(big, len(big), C.byref(bns), hout, hcap, None)
    assert hsize > 0 and payload == hout.raw[:hsize]
    n = C.c_int64(0)
    dsize = lib.mi355x_sam_to_bam_dev(big, len(big), C.byref(bns), out, cap, C.byref(n))
    assert dsize == hsize and out.raw[:dsize] == payload and n.value == big.count(b"\n")
    c = (C.c_uint64 * 6)()
    lib.mi355x_bam_dev_counts(c)
    assert c[0] == 2 * n.value and c[1] == 0   # both calls, every piece the device's
    lib.mi355x_finalize()
    print("three pieces: %d records, %d bytes of BAM" % (n.value, hsize))


if __name__ == "__main__":
    main()
