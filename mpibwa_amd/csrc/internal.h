// internal.h — shared declarations of the host side of libmpibwa_amd.so
#ifndef MBW_INTERNAL_H
#define MBW_INTERNAL_H

#include "../../include/mpibwa_amd.h"

#include <cstdint>
#include <cstddef>
#include <functional>
#include <string>
#include <vector>

namespace mbw {

[[noreturn]] void die(const char *fmt, ...);
void fill_cnt_table(uint32_t tab[256]);
extern const uint8_t *const nt4_table_ptr;
#define nt4_table nt4_table_ptr
// sampost.cpp: where the BGZF blocks of `len` bytes of text start and end (cut[0] = 0 .. cut[n_blocks] = len), the one rule of the host
// path and the device path (bgzf_stage.hip)
void bgzf_cuts(const char *text, size_t len, std::vector<size_t> &cut);
// sampost.cpp: the block table of `len` bytes of BGZF for both inflate paths (this host path and bgzf_in_stage.hip): blk_off[0 .. n] and
// text_off[0 .. n] as mi355x_bgzf_scan gives them; returns the offset at which the walk stopped short of len (a header that is not one,
// a block that the buffer cuts off), or -1 when the whole blocks end at len
int64_t bgzf_in_plan(const uint8_t *in, size_t len, std::vector<int64_t> &blk_off, std::vector<int64_t> &text_off);
// sampost.cpp, for both BAM paths (this host path and bam_stage.hip): the contig table of bam_util.h as one blob; the records of the
// whole lines of sam[0 .. len) into out (16 bytes of slack behind them) with their offsets (rec_off[0 .. n], rec_off[n] = the size),
// returns the size or -(offset of the first malformed line) - 1; and the blocks' cuts from those offsets
namespace bam { struct ContigTable; }
void bam_contig_blob(const bntseq_t *bns, std::vector<uint8_t> &blob);
int64_t bam_encode_host(const char *sam, size_t len, const bam::ContigTable &tab, std::vector<uint8_t> &out, std::vector<uint64_t> *rec_off);
void bam_cuts(const std::vector<uint64_t> &rec_off, std::vector<size_t> &cut);
// sampost.cpp, for bam_sort.cpp: f(lo, hi) over [0, n) in grains on the rank's host threads (MPIBWA_SAMPOST_THREADS); the blocks
// bytes[cut[b] .. cut[b + 1]) by zlib at `level` side by side into out (64 KiB per block are there), closed up; returns their size
void host_parallel(int64_t n, int64_t grain, const std::function<void(int64_t, int64_t)> &f);
size_t bgzf_blocks_at(const uint8_t *bytes, const std::vector<size_t> &cut, int level, uint8_t *out);
// bam_sort.cpp, for both sort paths (it and bam_sort_stage.hip): the records of the inflated stream s[h_end .. u) by one hop from record
// to record: their offsets, sizes (block_size's four bytes included) and packed keys (bam_sort_util.h); returns 0 or -(offset of the
// first malformed record) - 1
int64_t bam_sort_walk(const uint8_t *s, uint64_t h_end, uint64_t u, int32_t n_ref, std::vector<uint64_t> &off, std::vector<uint32_t> &size,
                      std::vector<uint64_t> &key);
// room for the sorted file of an inflated stream of u bytes (mi355x_bam_sort_bound); the cuts of the output stream: a new header of hn
// bytes in blocks of its own, then bam_cuts of the sorted records (rec_off[0 .. n] from 0) behind it
uint64_t bam_sort_bound_of(uint64_t u);
void bam_sort_cuts(uint64_t hn, const std::vector<uint64_t> &rec_off, std::vector<size_t> &cut);
// bam_index.cpp, for both index paths (it and bam_sort_stage.hip): the BAI index of a coordinate-sorted file on the host (the number of
// records, or -(offset) - 1 and bam_index_util.h's reason), and the bytes handed over as a malloc'ed buffer
int64_t bam_index_host(const uint8_t *bam, size_t len, std::vector<uint8_t> &bai, int *reason);
void bam_index_hand_over(const std::vector<uint8_t> &bai, uint8_t **out, size_t *out_len);

// ---- plain records exchanged between host stages and HIP kernels ----

struct Intv {            // bwtintv_t (src/bwt.h:60): bi-interval + (start<<32|end)
	uint64_t x0, x1, x2, info;
};

struct Seed {            // mem_seed_t (src/bwamem.c:168)
	int64_t rbeg;
	int32_t qbeg, len;
	int32_t score;
};

struct Chain {           // mem_chain_t (src/bwamem.c:174)
	int64_t pos;
	int rid;
	int first;
	uint32_t w;
	int kept;
	int is_alt;
	float frac_rep;
	std::vector<Seed> seeds;
};

struct AlnReg {          // mem_alnreg_t (src/bwamem.h:59), 88 bytes in the reference
	int64_t rb, re;
	int qb, qe;
	int rid;
	int score;
	int truesc;
	int sub;
	int alt_sc;
	int csub;
	int sub_n;
	int w;
	int seedcov;
	int secondary;
	int secondary_all;
	int seedlen0;
	int n_comp;
	int is_alt;
	float frac_rep;
	uint64_t hash;
};
typedef std::vector<AlnReg> AlnRegV;

struct Aln {             // mem_aln_t (src/bwamem.h:87)
	int64_t pos;
	int rid;
	int flag;
	uint32_t is_rev, is_alt, mapq, NM;
	int n_cigar;
	std::vector<uint32_t> cigar;
	std::string *unused;
	const char *XA;
	std::string md;
	int score, sub, alt_sc;
};

} // namespace mbw
#endif
