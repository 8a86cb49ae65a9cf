// sampost.cpp — what mpiBWA does with a chunk's SAM text between mem_process_seqs() and the file (the caller's
// side): `-f` fixmate, `-g` / `-b` BGZF output, and mpiBWAByChr's routing of records to per-contig files.  Host code, no MPI, no GPU:
// the text is the product of the hot path, these passes only re-arrange it.
//
//   fixmate        fixmate()                         src/fixmate.c:601-827   (per pair; parser :160-298, writers :374-599)
//                  call_fixmate                      src/parallel_aux.c:2164-2206   (the loop over a chunk's pairs)
//   BGZF           deflate_block                     src/bgzf.c:245-330      (one gzip member per block, 'BC' extra field)
//                  compress_and_write_bgzf_thread    src/parallel_aux.c:2941-3073   (-g: whole records per block)
//                  compress_and_write_bam_thread     src/parallel_aux.c:3075-3176   (-b: the same text; EOF block src/mainParallel.c:1509-1516)
//   by chromosome  the routing loops                 src/mainParallelByChromosome.c:1340-1455 (pairs), :3437-3486 (single end)
//                  getChr                            src/parallel_aux.c:2625-2648
//
// The reference's fixmate is restated record for record: the same three passes over the lines of a pair, the same fields and tags
// (MQ, MC, ms), the same order of the lines in each mate's text.  Where the reference's behaviour is undefined (it indexes the
// contig table with -1 when a supplementary line has RNEXT '*', and uses the tag text as a printf format) this file prints '*'
// and copies the tags literally.  The reference's compressed writers drop the last read of every thread's slice
// (`end_index = ... - 1`, src/parallel_aux.c:2953-2956) — here every record is written: the decompressed stream is the SAM text.
#include "internal.h"
#include "bam_util.h"

#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

using namespace mbw;

namespace {

enum : unsigned { F_PAIRED = 1, F_UNMAP = 4, F_MUNMAP = 8, F_REVERSE = 16, F_MREVERSE = 32, F_READ1 = 64, F_READ2 = 128, F_SECONDARY = 256, F_SUPP = 2048 };
constexpr int MIN_QUALITY = 15;   // MD_MIN_QUALITY (src/fixmate.h)

template <class F> void run_parallel(int64_t n, int64_t grain, F f)
{
	const int64_t n_blocks = (n + grain - 1) / grain;
	int n_thr = std::min(mi355x_host_cpus(), 32);
	if (const char *e = getenv("MPIBWA_SAMPOST_THREADS")) n_thr = std::max(1, std::min(atoi(e), 64));   // (the tests run the passes on 1, 3, ... threads)
	n_thr = (int)std::min<int64_t>(n_thr, n_blocks);
	if (n_thr <= 1) { for (int64_t b = 0; b < n_blocks; ++b) f(b * grain, std::min(n, (b + 1) * grain)); return; }
	std::atomic<int64_t> next(0);
	std::vector<std::thread> th;
	auto body = [&] { for (int64_t b; (b = next.fetch_add(1)) < n_blocks;) f(b * grain, std::min(n, (b + 1) * grain)); };
	for (int t = 1; t < n_thr; ++t) th.emplace_back(body);
	body();
	for (auto &t : th) t.join();
}

// contig name -> index, the first of equal names (the reference's linear search stops at the first match, src/fixmate.c:189-196)
struct ContigIndex {
	std::unordered_map<std::string_view, int> by_name;
	explicit ContigIndex(const bntseq_t *bns)
	{
		by_name.reserve((size_t)bns->n_seqs * 2);
		for (int i = 0; i < bns->n_seqs; ++i) by_name.emplace(std::string_view(bns->anns[i].name), i);
	}
	int find(std::string_view name) const
	{
		auto it = by_name.find(name);
		return it == by_name.end() ? -1 : it->second;
	}
};

// one SAM line of a pair, fields as views into the mate's text (readInfo, src/fixmate.h)
struct Rec {
	unsigned flag = 0;
	int tid = -1, mtid = -1;
	uint64_t pos = 0, mpos = 0;
	uint32_t mapq = 0, mmapq = 0, tlen = 0, score = 0, mscore = 0;
	std::string_view cigar, mcigar, seq, qual, aux;   // aux: everything behind the quality field, with the line's '\n'
	const char *name = nullptr;
	bool done = false;
};

std::string_view next_field(const char *&p, const char *end)
{
	const char *t = (const char *)memchr(p, '\t', (size_t)(end - p));
	std::string_view f(p, (size_t)((t ? t : end) - p));
	p = t ? t + 1 : end;
	return f;
}

int64_t to_int(std::string_view f)   // atoi / atol on a field (digits with an optional sign; anything else ends the number)
{
	size_t i = 0;
	bool neg = false;
	if (i < f.size() && (f[i] == '-' || f[i] == '+')) neg = f[i++] == '-';
	uint64_t v = 0;   // (unsigned: a field of twenty digits wraps around instead of overflowing a signed number)
	for (; i < f.size() && f[i] >= '0' && f[i] <= '9'; ++i) v = v * 10 + (uint64_t)(f[i] - '0');
	return (int64_t)(neg ? 0 - v : v);
}

// readParsing (src/fixmate.c:160-298): [line, line_end) holds one record without its '\n'; `tail_end` is behind the '\n'
bool parse_line(const char *line, const char *line_end, const char *tail_end, const ContigIndex &ci, Rec &r)
{
	const char *p = line;
	next_field(p, line_end);                                   // QNAME: the caller's bseq1_t::name is printed instead
	r.flag = (unsigned)to_int(next_field(p, line_end));
	if (r.flag == 0) return false;                             // (the reference asserts a non-zero flag)
	r.tid = ci.find(next_field(p, line_end));
	const std::string_view pos = next_field(p, line_end);
	r.pos = pos == "*" ? (uint64_t)-1 : (uint64_t)to_int(pos);
	r.mapq = (uint32_t)to_int(next_field(p, line_end));
	r.cigar = next_field(p, line_end);
	const std::string_view rnext = next_field(p, line_end);
	r.mtid = rnext == "=" ? r.tid : ci.find(rnext);
	const std::string_view mpos = next_field(p, line_end);
	r.mpos = mpos == "*" ? (uint64_t)-1 : (uint64_t)to_int(mpos);
	r.tlen = (uint32_t)to_int(next_field(p, line_end));
	r.seq = next_field(p, line_end);
	r.qual = next_field(p, line_end);
	for (const char c : r.qual)
		if (c - 33 >= MIN_QUALITY) r.score += (uint32_t)(c - 33);
	r.aux = std::string_view(p, (size_t)(tail_end - p));       // the tags and the newline ("\n" alone when there are none)
	return true;
}

struct Out {
	std::string s;
	void str(std::string_view v) { s.append(v.data(), v.size()); }
	void tab() { s.push_back('\t'); }
	void u64(uint64_t v) { char b[24]; s.append(b, (size_t)snprintf(b, sizeof b, "%llu", (unsigned long long)v)); }
	void i32(int v) { char b[16]; s.append(b, (size_t)snprintf(b, sizeof b, "%d", v)); }
	void u32(uint32_t v) { char b[16]; s.append(b, (size_t)snprintf(b, sizeof b, "%u", v)); }
};

const char *contig(const bntseq_t *bns, int tid) { return tid >= 0 && tid < bns->n_seqs ? bns->anns[tid].name : "*"; }

// the eleven mandatory fields, as every writer of src/fixmate.c prints them (name, flag, RNAME, POS, MAPQ, CIGAR, RNEXT, PNEXT, TLEN, SEQ, QUAL)
void put_core(Out &o, const Rec &r, const char *chr, const char *mchr)
{
	o.str(r.name); o.tab(); o.i32((int)r.flag); o.tab(); o.str(chr); o.tab(); o.u64(r.pos); o.tab(); o.i32((int)r.mapq); o.tab();
	o.str(r.cigar); o.tab(); o.str(mchr); o.tab(); o.u64(r.mpos); o.tab(); o.i32((int)r.tlen); o.tab(); o.str(r.seq); o.tab(); o.str(r.qual); o.tab();
}

// sam_write_unmapped_and_munmapped (src/fixmate.c:447-495)
void write_both_unmapped(Out &o, const Rec &r, const bntseq_t *bns)
{
	const char *chr, *mchr = nullptr;
	if (r.tid == -1 && r.mtid == -1) { chr = "*"; mchr = "*"; }
	else chr = contig(bns, r.tid);
	if (r.tid != -1 && r.tid == r.mtid) mchr = "=";
	if (r.mtid != -1) mchr = contig(bns, r.mtid);
	if (!mchr) mchr = "*";
	put_core(o, r, chr, mchr);
	o.str("ms:i:"); o.u32(r.mscore); o.tab(); o.str(r.aux);
}
// sam_write (src/fixmate.c:549-597): both ends mapped, same contig or not decided by the caller
void write_pair(Out &o, const Rec &r, const bntseq_t *bns)
{
	put_core(o, r, contig(bns, r.tid), r.tid == r.mtid ? "=" : contig(bns, r.mtid));
	o.str("MQ:i:"); o.i32((int)r.mmapq); o.tab(); o.str("ms:i:"); o.u32(r.mscore); o.tab(); o.str(r.aux);
}
// sam_write_discordant (src/fixmate.c:406-443): the mate's contig by name, MQ + MC + ms
void write_discordant(Out &o, const Rec &r, const bntseq_t *bns)
{
	put_core(o, r, contig(bns, r.tid), contig(bns, r.mtid));
	o.str("MQ:i:"); o.i32((int)r.mmapq); o.tab(); o.str("MC:Z:"); o.str(r.mcigar); o.tab(); o.str("ms:i:"); o.u32(r.mscore); o.tab(); o.str(r.aux);
}
// sam_write_mate_unmapped (src/fixmate.c:497-547): one end of the pair is unmapped
void write_one_unmapped(Out &o, const Rec &r, const bntseq_t *bns)
{
	put_core(o, r, contig(bns, r.tid), r.tid == r.mtid ? "=" : contig(bns, r.mtid));
	if (r.flag & F_UNMAP) { o.str("MQ:i:"); o.i32((int)r.mmapq); o.tab(); o.str("MC:Z:"); o.str(r.mcigar); o.tab(); }
	else o.str("MC:Z:*\t");
	o.str("ms:i:"); o.u32(r.mscore); o.tab(); o.str(r.aux);
}
// sam_write_supp_and_secondary (src/fixmate.c:374-404): the mate's contig by name, no tags added
void write_supp(Out &o, const Rec &r, const bntseq_t *bns)
{
	put_core(o, r, contig(bns, r.tid), contig(bns, r.mtid));
	o.str(r.aux);
}

// sync_mate (src/fixmate.c:317-366)
void sync_one_way(const Rec &src, Rec &dst)
{
	dst.mtid = src.tid; dst.mpos = src.pos;
	if (src.flag & F_REVERSE) dst.flag |= F_MREVERSE; else dst.flag &= ~(unsigned)F_MREVERSE;
	if (src.flag & F_UNMAP) dst.flag |= F_MUNMAP;
}
void sync_mate(Rec &a, Rec &b)
{
	if ((b.flag & F_UNMAP) && !(a.flag & F_UNMAP)) { b.tid = a.tid; b.pos = a.pos; }
	if ((a.flag & F_UNMAP) && !(b.flag & F_UNMAP)) { a.tid = b.tid; a.pos = b.pos; }
	sync_one_way(a, b);
	sync_one_way(b, a);
	if (!(a.flag & F_UNMAP)) { b.mmapq = a.mapq; b.mcigar = a.cigar; }
	if (!(b.flag & F_UNMAP)) { a.mmapq = b.mapq; a.mcigar = b.cigar; }
}

// the lines of one mate's text -> recs; false when a line does not parse
bool split_lines(const bseq1_t &s, const ContigIndex &ci, std::vector<Rec> &recs, int &n_lines)
{
	n_lines = 0;
	if (!s.sam) return true;
	const char *p = s.sam, *end = p + strlen(p);
	while (p < end) {
		const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
		if (!nl) break;   // (the reference's line reader stops at text without a newline too: src/fixmate.c:301-315)
		Rec r;
		r.name = s.name ? s.name : "";
		if (!parse_line(p, nl, nl + 1, ci, r)) return false;
		recs.push_back(r);
		++n_lines;
		p = nl + 1;
	}
	return true;
}

int fixmate_pair(bseq1_t *s1, bseq1_t *s2, const bntseq_t *bns, const ContigIndex &ci, std::vector<Rec> &recs, Out o[2])
{
	recs.clear(); o[0].s.clear(); o[1].s.clear();
	int n1 = 0, n2 = 0;
	if (!split_lines(*s1, ci, recs, n1) || !split_lines(*s2, ci, recs, n2)) return -1;
	const int n = n1 + n2;
	Rec *r1 = nullptr, *r2 = nullptr;
	int have = 0;
	auto take = [&](Rec &r) {
		if (r.flag & F_READ1) { r1 = &r; ++have; }
		if (r.flag & F_READ2) { r2 = &r; ++have; }
		return have == 2 && r1 && r2;
	};
	// pass 1: both ends unmapped (src/fixmate.c:693-718)
	for (int i = 0; i < n; ++i) {
		Rec &r = recs[i];
		if (r.done || !(r.flag & F_UNMAP) || !(r.flag & F_MUNMAP)) continue;
		if (!take(r)) continue;
		r1->flag |= F_PAIRED; r2->flag |= F_PAIRED;
		r2->mscore = r1->score; r1->mscore = r2->score;
		write_both_unmapped(o[0], *r1, bns); write_both_unmapped(o[1], *r2, bns);
		r1->done = r2->done = true; have = 0;
	}
	// pass 2: the primary lines of a pair with both ends mapped (src/fixmate.c:721-773)
	have = 0;
	for (int i = 0; i < n; ++i) {
		Rec &r = recs[i];
		if (r.done || !(r.flag & F_PAIRED) || (r.flag & (F_SECONDARY | F_SUPP | F_UNMAP | F_MUNMAP))) continue;
		if (!take(r)) continue;
		const bool other_contigs = r1->tid != r1->mtid && r2->tid != r2->mtid;   // (as the lines came in, before the mates are synchronised)
		sync_mate(*r1, *r2);
		r2->mscore = r1->score; r1->mscore = r2->score;
		if (other_contigs) { write_discordant(o[0], *r1, bns); write_discordant(o[1], *r2, bns); }
		else { write_pair(o[0], *r1, bns); write_pair(o[1], *r2, bns); }
		r1->done = r2->done = true; have = 0;
	}
	// pass 3: secondary and supplementary lines as they come, and the pair with one end unmapped (src/fixmate.c:775-808)
	have = 0;
	for (int i = 0; i < n; ++i) {
		Rec &r = recs[i];
		if (r.done) continue;
		if (r.flag & (F_SECONDARY | F_SUPP)) { write_supp(o[(r.flag & F_READ1) ? 0 : 1], r, bns); r.done = true; continue; }
		if (!(r.flag & F_PAIRED)) continue;
		if (!take(r)) continue;
		sync_mate(*r1, *r2);
		r2->mscore = r1->score; r1->mscore = r2->score;
		write_one_unmapped(o[0], *r1, bns); write_one_unmapped(o[1], *r2, bns);
		r1->done = r2->done = true; have = 0;
	}
	for (int i = 0; i < n; ++i)
		if (!recs[i].done) return -1;   // (the reference asserts that no line is left over, src/fixmate.c:810)
	if (o[0].s.empty() || o[1].s.empty()) return -1;
	char *t1 = (char *)malloc(o[0].s.size() + 1), *t2 = (char *)malloc(o[1].s.size() + 1);
	if (!t1 || !t2) die("out of memory in fixmate");
	memcpy(t1, o[0].s.c_str(), o[0].s.size() + 1);
	memcpy(t2, o[1].s.c_str(), o[1].s.size() + 1);
	free(s1->sam); free(s2->sam);   // (recs' views die here)
	s1->sam = t1; s2->sam = t2;
	return n;
}

// ---- BGZF ----
constexpr size_t BGZF_INPUT = 0xff00;     // text per block: what always fits a 64-KiB block, stored (htslib's choice; src/bgzf.c: 64 KiB, shrinking on overflow)
constexpr size_t BGZF_HEAD = 18, BGZF_TAIL = 8, BGZF_MAX = 0x10000;

// one block (src/bgzf.c:245-330): gzip header with the 'BC' extra field (total block size - 1), raw deflate, CRC32, input length
size_t bgzf_block(const uint8_t *in, size_t n, int level, uint8_t *out)
{
	static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
	size_t clen = 0;
	for (int attempt = 0; attempt < 2; ++attempt) {
		z_stream zs;
		memset(&zs, 0, sizeof zs);
		if (deflateInit2(&zs, attempt ? 0 : level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) die("BGZF: deflateInit2 failed");
		zs.next_in = (Bytef *)in; zs.avail_in = (uInt)n;
		zs.next_out = out + BGZF_HEAD; zs.avail_out = (uInt)(BGZF_MAX - BGZF_HEAD - BGZF_TAIL);
		const int rc = deflate(&zs, Z_FINISH);
		clen = zs.total_out;
		deflateEnd(&zs);
		if (rc == Z_STREAM_END) break;
		if (attempt) die("BGZF: a block of %zu bytes does not fit 64 KiB", n);   // (level 0 always fits BGZF_INPUT bytes)
	}
	memcpy(out, head, 16);
	const size_t total = BGZF_HEAD + clen + BGZF_TAIL;
	out[16] = (uint8_t)((total - 1) & 0xff); out[17] = (uint8_t)((total - 1) >> 8);
	const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, (uInt)n), isize = (uint32_t)n;
	uint8_t *t = out + BGZF_HEAD + clen;
	for (int k = 0; k < 4; ++k) { t[k] = (uint8_t)(crc >> (8 * k)); t[4 + k] = (uint8_t)(isize >> (8 * k)); }
	return total;
}

} // namespace

// ---- fixmate ----
// One pair (src/fixmate.c:601): s1->sam / s2->sam are replaced (malloc family, the caller frees them as before).  Returns the
// number of SAM lines of the pair, or -1 when the text is not what mem_sam_pe writes for a pair (a line without a flag, lines left
// over after the three passes): the texts are then left as they were.
extern "C" int mi355x_fixmate_pair(bseq1_t *s1, bseq1_t *s2, const bntseq_t *bns)
{
	const ContigIndex ci(bns);
	std::vector<Rec> recs;
	Out o[2];
	return fixmate_pair(s1, s2, bns, ci, recs, o);
}

// All pairs of a chunk (call_fixmate, src/parallel_aux.c:2164-2206), on the host threads of this rank.  Returns the number of SAM
// lines, or -(index of the first read of the pair that failed) - 1.
extern "C" int64_t mi355x_fixmate(bseq1_t *seqs, int n, const bntseq_t *bns)
{
	if (n & 1) die("mi355x_fixmate: %d reads are not pairs", n);
	const ContigIndex ci(bns);
	std::atomic<int64_t> lines(0), bad(-1);
	run_parallel(n / 2, 2048, [&](int64_t lo, int64_t hi) {
		std::vector<Rec> recs;
		Out o[2];
		int64_t mine = 0;
		for (int64_t p = lo; p < hi; ++p) {
			const int k = fixmate_pair(&seqs[2 * p], &seqs[2 * p + 1], bns, ci, recs, o);
			if (k < 0) { int64_t none = -1; bad.compare_exchange_strong(none, 2 * p); continue; }
			mine += k;
		}
		lines += mine;
	});
	return bad.load() >= 0 ? -bad.load() - 1 : lines.load();
}

// run_parallel for the host files beside this one (bam_sort.cpp): the same threads, the same MPIBWA_SAMPOST_THREADS
void mbw::host_parallel(int64_t n, int64_t grain, const std::function<void(int64_t, int64_t)> &f) { run_parallel(n, grain, f); }

// ---- BGZF ----
// The cuts of both BGZF paths (this file's and the device's, bgzf_stage.hip): at most BGZF_INPUT bytes per block, cut back to the last
// record end where there is one.
void mbw::bgzf_cuts(const char *text, size_t len, std::vector<size_t> &cut)
{
	cut.assign(1, 0);
	for (size_t at = 0; at < len;) {
		size_t n = std::min(BGZF_INPUT, len - at);
		if (at + n < len) {
			const void *nl = memrchr(text + at, '\n', n);
			if (nl) n = (size_t)((const char *)nl - (text + at)) + 1;
		}
		at += n;
		cut.push_back(at);
	}
}

// room for the compressed form of `len` bytes of text
extern "C" size_t mi355x_bgzf_bound(size_t len) { return (len / (BGZF_INPUT / 2) + 2) * BGZF_MAX; }

// `len` bytes of SAM text as BGZF blocks into out[cap]: blocks end at record ends where a record fits a block (the reference's -g
// writer packs whole reads' records, src/parallel_aux.c:3003-3017), the blocks are compressed side by side and the result does
// not depend on the number of threads.  level: zlib's (-1 = default, as src/bgzf.c:95).  Returns the compressed size, 0 when cap is
// too small.
// the blocks bytes[cut[b] .. cut[b + 1]) side by side into out (n_blocks * BGZF_MAX bytes are there), closed up; returns their size
size_t mbw::bgzf_blocks_at(const uint8_t *bytes, const std::vector<size_t> &cut, int level, uint8_t *out)
{
	const size_t n_blocks = cut.size() - 1;
	std::vector<uint32_t> clen(n_blocks);
	// every block into its own 64-KiB slot, then the slots are closed up
	run_parallel((int64_t)n_blocks, 16, [&](int64_t lo, int64_t hi) {
		for (int64_t b = lo; b < hi; ++b) clen[b] = (uint32_t)bgzf_block(bytes + cut[b], cut[b + 1] - cut[b], level, out + (size_t)b * BGZF_MAX);
	});
	size_t w = 0;
	for (size_t b = 0; b < n_blocks; ++b) { memmove(out + w, out + b * BGZF_MAX, clen[b]); w += clen[b]; }
	return w;
}

extern "C" size_t mi355x_bgzf_compress(const char *text, size_t len, int level, uint8_t *out, size_t cap)
{
	if (level > 9 || level < 0) level = Z_DEFAULT_COMPRESSION;
	std::vector<size_t> cut;
	bgzf_cuts(text, len, cut);
	const size_t n_blocks = cut.size() - 1;
	if (n_blocks * BGZF_MAX > cap) return 0;
	return bgzf_blocks_at((const uint8_t *)text, cut, level, out);
}

// the empty block that ends a BGZF file (src/mainParallel.c:1510: the 28 bytes the reference appends to its .bam)
extern "C" size_t mi355x_bgzf_eof(uint8_t out[28])
{
	static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	memcpy(out, eof, 28);
	return 28;
}

// ---- BGZF input ----
// Is there a BGZF block header at p (18 bytes are there)?  1f 8b 08 04, six bytes that any writer may fill (MTIME, XFL, OS), XLEN = 6,
// the 'BC' field of two bytes, and a BSIZE that leaves room for the header and the trailer.  Returns the block's size or 0.
static inline int64_t bgzf_header_at(const uint8_t *p)
{
	if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4 || p[10] != 6 || p[11] != 0 || p[12] != 'B' || p[13] != 'C' || p[14] != 2 || p[15] != 0) return 0;
	const int64_t total = (int64_t)(p[16] | p[17] << 8) + 1;
	return total >= (int64_t)(BGZF_HEAD + BGZF_TAIL) ? total : 0;
}

// The first offset of buf[0 .. len) at which a BGZF block starts, for a rank that enters a file in the middle; at_eof: buf ends where
// the file ends.  -1: none; -2: the first candidate cannot be decided without more bytes.
// The ten fixed bytes of a header do occur inside compressed payload (and a stored block can hold any bytes, a BGZF file for one), so a
// header alone is no start.  A start is a header from which the BSIZE hops meet TWO more headers (or the end of the file exactly):
// three headers are 30 fixed bytes at places that the first two name, which no payload has by accident; one more link would not help
// against a payload built on purpose (a stored block can carry a chain of any length), and the inflate's CRC catches that case.
extern "C" int64_t mi355x_bgzf_find_block(const uint8_t *buf, int64_t len, int at_eof)
{
	for (int64_t o = 0; o < len; ++o) {
		if (buf[o] != 0x1f) continue;
		int64_t at = o;
		int links = 0;
		for (; links < 3; ++links) {
			if (at == len && at_eof && links > 0) { links = 3; break; }
			if (at + (int64_t)BGZF_HEAD > len) {
				if (!at_eof) return -2;
				break;
			}
			const int64_t total = bgzf_header_at(buf + at);
			if (!total) break;
			at += total;
		}
		if (links == 3) return o;
	}
	return -1;
}

// The headers of buf[0 .. len) from offset 0, at most cap blocks: blk_off[i] = where block i starts, blk_off[n] = where the last whole
// block ends; text_off[i] = the ISIZEs of the blocks before i, text_off[n] = the text's size (both arrays: cap + 1 entries).  Returns n,
// or -(offset) - 1 of 18 bytes that are no header or of a block whose ISIZE is above 64 KiB.  A block that buf cuts off ends the walk
// without an error.  Blocks of ISIZE 0 (the 28-byte EOF block, wherever it stands) are blocks like any other.
extern "C" int64_t mi355x_bgzf_scan(const uint8_t *buf, int64_t len, int64_t cap, int64_t *blk_off, int64_t *text_off)
{
	int64_t n = 0, at = 0, text = 0;
	blk_off[0] = 0; text_off[0] = 0;
	while (n < cap && at + (int64_t)BGZF_HEAD <= len) {
		const int64_t total = bgzf_header_at(buf + at);
		if (!total) return -at - 1;
		if (at + total > len) break;
		const uint8_t *t = buf + at + total - 4;
		const int64_t isize = (int64_t)((uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24);
		if (isize > (int64_t)BGZF_MAX) return -at - 1;
		at += total; text += isize; ++n;
		blk_off[n] = at; text_off[n] = text;
	}
	return n;
}

int64_t mbw::bgzf_in_plan(const uint8_t *in, size_t len, std::vector<int64_t> &blk_off, std::vector<int64_t> &text_off)
{
	const int64_t cap = (int64_t)(len / (BGZF_HEAD + BGZF_TAIL)) + 1;
	blk_off.resize((size_t)cap + 1); text_off.resize((size_t)cap + 1);
	int64_t n = mi355x_bgzf_scan(in, (int64_t)len, cap, blk_off.data(), text_off.data());
	int64_t bad = -1;
	if (n < 0) {   // the blocks before the bad header still count: one of them may fail first
		bad = -n - 1;
		n = bad ? mi355x_bgzf_scan(in, bad, cap, blk_off.data(), text_off.data()) : 0;
	} else if ((size_t)blk_off[n] != len) bad = blk_off[n];
	blk_off.resize((size_t)n + 1); text_off.resize((size_t)n + 1);
	return bad;
}

// `len` bytes of whole BGZF blocks to their text in out[cap], a block per task on this rank's host threads (zlib's raw inflate); every
// block's CRC32 and ISIZE are checked.  Returns the text's size, -(offset of the first block that fails) - 1, or 0 with nothing written
// when cap is smaller than the text.  No GPU.
extern "C" int64_t mi355x_bgzf_inflate(const uint8_t *in, size_t len, char *out, size_t cap)
{
	std::vector<int64_t> blk, txt;
	const int64_t bad = bgzf_in_plan(in, len, blk, txt);
	const int64_t n = (int64_t)blk.size() - 1;
	if ((uint64_t)txt[n] > cap) return 0;
	std::atomic<int64_t> first_bad(INT64_MAX);
	run_parallel(n, 16, [&](int64_t lo, int64_t hi) {
		for (int64_t b = lo; b < hi; ++b) {
			const uint8_t *p = in + blk[b];
			const size_t total = (size_t)(blk[b + 1] - blk[b]), isize = (size_t)(txt[b + 1] - txt[b]);
			const uint8_t *t = p + total - 8;
			const uint32_t crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
			z_stream zs;
			memset(&zs, 0, sizeof zs);
			bool ok = inflateInit2(&zs, -15) == Z_OK;
			if (ok) {
				uint8_t none = 0;
				zs.next_in = (Bytef *)(p + BGZF_HEAD); zs.avail_in = (uInt)(total - BGZF_HEAD - BGZF_TAIL);
				zs.next_out = isize ? (Bytef *)out + txt[b] : &none; zs.avail_out = (uInt)isize;
				ok = inflate(&zs, Z_FINISH) == Z_STREAM_END && zs.total_out == isize;
				inflateEnd(&zs);
				ok = ok && (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)out + txt[b], (uInt)isize) == crc;
			}
			if (!ok) {
				int64_t cur = first_bad.load();
				while (blk[b] < cur && !first_bad.compare_exchange_weak(cur, blk[b])) {}
			}
		}
	});
	if (first_bad.load() != INT64_MAX) return -first_bad.load() - 1;
	if (bad >= 0) return -bad - 1;
	return txt[n];
}

// ---- mpiBWAByChr's routing ----
// The records of `sam` (len bytes, whole lines) by destination: 0 .. n_seqs-1 = the contig named in RNAME, then "discordant" (only
// when discordant != 0: pairs without -f, src/mainParallelByChromosome.c:986-1004), last "unmapped" (RNAME '*').  A record whose
// RNAME and RNEXT are two different contigs goes to its contig AND to "discordant" (:1437-1441).  out_text[d] (malloc, or NULL when
// nothing goes there) / out_len[d] for d < n_seqs + 1 + (discordant != 0); record order is kept inside every destination.
// Returns the number of records, or -(byte offset) - 1 of a line that has no RNAME field.
extern "C" int64_t mi355x_route_by_chr(const char *sam, size_t len, const bntseq_t *bns, int discordant, char **out_text, size_t *out_len)
{
	const ContigIndex ci(bns);
	const int n_dest = bns->n_seqs + 1 + (discordant ? 1 : 0), d_unmapped = n_dest - 1, d_disc = discordant ? bns->n_seqs : -1;
	struct Line { size_t at; uint32_t n; int dest; bool disc; };
	// the text in segments of whole lines, parsed side by side; a destination's records keep the order of the text (segment by segment)
	struct Seg { size_t lo = 0, hi = 0; std::vector<Line> lines; std::vector<size_t> bytes; int64_t bad = -1; };
	constexpr size_t SEG = 4u << 20;
	std::vector<Seg> segs;
	for (size_t at = 0; at < len;) {
		size_t hi = std::min(len, at + SEG);
		if (hi < len) {
			const void *nl = memchr(sam + hi, '\n', len - hi);
			hi = nl ? (size_t)((const char *)nl - sam) + 1 : len;
		}
		Seg g;
		g.lo = at; g.hi = hi;
		segs.push_back(std::move(g));
		at = hi;
	}
	run_parallel((int64_t)segs.size(), 1, [&](int64_t s0, int64_t s1) {
		for (int64_t si = s0; si < s1; ++si) {
			Seg &g = segs[(size_t)si];
			g.bytes.assign((size_t)n_dest, 0);
			g.lines.reserve((g.hi - g.lo) / 200 + 16);
			for (size_t at = g.lo; at < g.hi;) {
				const char *p = sam + at, *end = sam + g.hi;
				const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
				const char *le = nl ? nl : end;
				const size_t n = (size_t)(le - p) + (nl ? 1 : 0);
				const char *q = p;
				next_field(q, le); next_field(q, le);
				if (q >= le) { g.bad = (int64_t)at; return; }
				const std::string_view rname = next_field(q, le);
				Line L{at, (uint32_t)n, d_unmapped, false};
				if (rname != "*") {
					const int chr = ci.find(rname);
					if (chr >= 0) {
						L.dest = chr;
						if (discordant) {
							next_field(q, le); next_field(q, le); next_field(q, le);   // POS, MAPQ, CIGAR
							const std::string_view rnext = next_field(q, le);
							const int mchr = rnext == "=" ? chr : rnext == "*" ? -1 : ci.find(rnext);
							L.disc = mchr >= 0 && mchr != chr;
						}
					}
				}
				g.bytes[(size_t)L.dest] += n;
				if (L.disc) g.bytes[(size_t)d_disc] += n;
				g.lines.push_back(L);
				at += n;
			}
		}
	});
	int64_t n_lines = 0;
	std::vector<size_t> total((size_t)n_dest, 0);
	for (Seg &g : segs) {
		if (g.bad >= 0) return -g.bad - 1;
		n_lines += (int64_t)g.lines.size();
		for (int d = 0; d < n_dest; ++d) { const size_t b = g.bytes[(size_t)d]; g.bytes[(size_t)d] = total[(size_t)d]; total[(size_t)d] += b; }   // -> where the segment's records start
	}
	for (int d = 0; d < n_dest; ++d) {
		out_len[d] = total[(size_t)d];
		out_text[d] = nullptr;
		if (total[(size_t)d]) {
			out_text[d] = (char *)malloc(total[(size_t)d] + 1);
			if (!out_text[d]) die("out of memory routing SAM records");
			out_text[d][total[(size_t)d]] = 0;
		}
	}
	run_parallel((int64_t)segs.size(), 1, [&](int64_t s0, int64_t s1) {
		for (int64_t si = s0; si < s1; ++si) {
			Seg &g = segs[(size_t)si];
			for (const Line &L : g.lines) {
				memcpy(out_text[L.dest] + g.bytes[(size_t)L.dest], sam + L.at, L.n); g.bytes[(size_t)L.dest] += L.n;
				if (L.disc) { memcpy(out_text[d_disc] + g.bytes[(size_t)d_disc], sam + L.at, L.n); g.bytes[(size_t)d_disc] += L.n; }
			}
		}
	});
	return n_lines;
}

// ---- BAM records (bam_util.h) ----
// The contig table of bam_util.h: the names sorted, equal names by index.
void mbw::bam_contig_blob(const bntseq_t *bns, std::vector<uint8_t> &blob)
{
	const int n = bns->n_seqs;
	std::vector<int32_t> order((size_t)n);
	for (int i = 0; i < n; ++i) order[(size_t)i] = i;
	std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
		const char *x = bns->anns[a].name, *y = bns->anns[b].name;
		const int c = bam::name_cmp((const uint8_t *)x, (uint32_t)strlen(x), (const uint8_t *)y, (uint32_t)strlen(y));
		return c ? c < 0 : a < b;
	});
	size_t bytes = 0;
	for (int i = 0; i < n; ++i) bytes += strlen(bns->anns[i].name);
	blob.assign(4 + 4 * (size_t)n + 4 * ((size_t)n + 1) + bytes, 0);
	int32_t *w = (int32_t *)blob.data();
	w[0] = n;
	uint32_t *off = (uint32_t *)(w + 1 + n);
	uint8_t *names = (uint8_t *)(off + n + 1);
	uint32_t at = 0;
	for (int k = 0; k < n; ++k) {
		const char *nm = bns->anns[order[(size_t)k]].name;
		const uint32_t l = (uint32_t)strlen(nm);
		w[1 + k] = order[(size_t)k];
		off[k] = at;
		memcpy(names + at, nm, l);
		at += l;
	}
	off[n] = at;
}

namespace {

struct BamSeg {
	size_t lo = 0, hi = 0;
	std::vector<size_t> at;               // where every line starts
	std::vector<bam::LinePlan> plan;
	uint64_t bytes = 0, base = 0;         // of the segment's records; where they start in the stream
	int64_t bad = -1;
};

// The size pass over the whole lines of sam[0 .. len) in segments, side by side.  Returns the records' bytes, or -(offset) - 1 of the
// first malformed line (a last line without '\n' is one).
int64_t bam_plan(const char *sam, size_t len, const bam::ContigTable &tab, std::vector<BamSeg> &segs, int64_t &n_records)
{
	constexpr size_t SEG = 4u << 20;
	const void *last_nl = len ? memrchr(sam, '\n', len) : nullptr;
	const size_t body = last_nl ? (size_t)((const char *)last_nl - sam) + 1 : 0;   // the whole lines
	segs.clear();
	for (size_t at = 0; at < body;) {
		size_t hi = std::min(body, at + SEG);
		if (hi < body) hi = (size_t)((const char *)memchr(sam + hi - 1, '\n', body - hi + 1) - sam) + 1;
		BamSeg g;
		g.lo = at; g.hi = hi;
		segs.push_back(std::move(g));
		at = hi;
	}
	run_parallel((int64_t)segs.size(), 1, [&](int64_t s0, int64_t s1) {
		for (int64_t si = s0; si < s1; ++si) {
			BamSeg &g = segs[(size_t)si];
			g.at.reserve((g.hi - g.lo) / 200 + 16);
			g.plan.reserve((g.hi - g.lo) / 200 + 16);
			for (size_t at = g.lo; at < g.hi;) {
				const char *nl = (const char *)memchr(sam + at, '\n', g.hi - at);
				const size_t n = (size_t)(nl - (sam + at));
				bam::LinePlan P;
				if (n > 0xffffffffu || bam::plan_line((const uint8_t *)sam + at, (uint32_t)n, tab, P) != bam::BAM_OK) { g.bad = (int64_t)at; break; }
				g.at.push_back(at);
				g.plan.push_back(P);
				g.bytes += P.size;
				at += n + 1;
			}
		}
	});
	uint64_t total = 0;
	n_records = 0;
	for (BamSeg &g : segs) {
		if (g.bad >= 0) return -g.bad - 1;
		g.base = total;
		total += g.bytes;
		n_records += (int64_t)g.plan.size();
	}
	if (body < len) return -(int64_t)body - 1;
	return (int64_t)total;
}

void bam_write(const char *sam, const std::vector<BamSeg> &segs, uint8_t *out)
{
	run_parallel((int64_t)segs.size(), 1, [&](int64_t s0, int64_t s1) {
		for (int64_t si = s0; si < s1; ++si) {
			const BamSeg &g = segs[(size_t)si];
			uint64_t w = g.base;
			for (size_t k = 0; k < g.plan.size(); ++k) {
				bam::write_record((const uint8_t *)sam + g.at[k], g.plan[k], out + w);
				w += g.plan[k].size;
			}
		}
	});
}

void bam_offsets(const std::vector<BamSeg> &segs, std::vector<uint64_t> &off)
{
	off.clear();
	uint64_t w = 0;
	for (const BamSeg &g : segs)
		for (const bam::LinePlan &P : g.plan) { off.push_back(w); w += P.size; }
	off.push_back(w);
}

} // namespace

// The cuts of both BAM paths from the records' offsets (off[0 .. n], off[n] = the stream's size): bam::last_fit's rule; a record
// that alone is larger than a block is cut into blocks of BGZF_INPUT bytes, as bgzf_cuts cuts a line without a newline in reach.
void mbw::bam_cuts(const std::vector<uint64_t> &off, std::vector<size_t> &cut)
{
	const uint32_t n = (uint32_t)(off.size() - 1);
	cut.assign(1, 0);
	for (uint32_t i = 0; i < n;) {
		const uint32_t j = bam::last_fit(off.data(), n, i);
		if (j > i) { cut.push_back((size_t)off[j]); i = j; continue; }
		for (uint64_t at = off[i]; at < off[i + 1];) {   // the oversized record alone
			at = std::min(off[i + 1], at + BGZF_INPUT);
			cut.push_back((size_t)at);
		}
		++i;
	}
}

int64_t mbw::bam_encode_host(const char *sam, size_t len, const bam::ContigTable &tab, std::vector<uint8_t> &out, std::vector<uint64_t> *rec_off)
{
	std::vector<BamSeg> segs;
	int64_t n_rec = 0;
	const int64_t total = bam_plan(sam, len, tab, segs, n_rec);
	if (total < 0) return total;
	out.resize((size_t)total + 16);   // (slack for the device deflate's dword loads)
	bam_write(sam, segs, out.data());
	if (rec_off) bam_offsets(segs, *rec_off);
	return total;
}

// "BAM\1", the header text, the contigs of bns (include/mpibwa_amd.h)
extern "C" int64_t mi355x_bam_header(const char *text, size_t len, const bntseq_t *bns, uint8_t *out, size_t cap)
{
	size_t need = 4 + 4 + len + 4;
	for (int i = 0; i < bns->n_seqs; ++i) need += 4 + strlen(bns->anns[i].name) + 1 + 4;
	if (need > cap) return 0;
	uint8_t *w = out;
	memcpy(w, "BAM\1", 4); w += 4;
	bam::put32(w, (uint32_t)len); w += 4;
	if (len) memcpy(w, text, len);
	w += len;
	bam::put32(w, (uint32_t)bns->n_seqs); w += 4;
	for (int i = 0; i < bns->n_seqs; ++i) {
		const uint32_t l = (uint32_t)strlen(bns->anns[i].name) + 1;
		bam::put32(w, l); w += 4;
		memcpy(w, bns->anns[i].name, l); w += l;
		bam::put32(w, (uint32_t)bns->anns[i].len); w += 4;
	}
	return (int64_t)need;
}

extern "C" int64_t mi355x_bam_bound(size_t sam_len) { return (int64_t)bam::records_bound(sam_len); }

extern "C" int64_t mi355x_sam_to_bam(const char *sam, size_t len, const bntseq_t *bns, uint8_t *out, size_t cap, int64_t *n_records)
{
	std::vector<uint8_t> blob;
	bam_contig_blob(bns, blob);
	std::vector<BamSeg> segs;
	int64_t n_rec = 0;
	const int64_t total = bam_plan(sam, len, bam::contig_table_at(blob.data()), segs, n_rec);
	if (total < 0) return total;
	if ((uint64_t)total > cap) return 0;
	bam_write(sam, segs, out);
	if (n_records) *n_records = n_rec;
	return total;
}

extern "C" int64_t mi355x_bam_compress(const char *sam, size_t len, const bntseq_t *bns, int level, uint8_t *out, size_t cap)
{
	if (level > 9 || level < 0) level = Z_DEFAULT_COMPRESSION;
	std::vector<uint8_t> blob, recs;
	bam_contig_blob(bns, blob);
	std::vector<uint64_t> off;
	const int64_t total = bam_encode_host(sam, len, bam::contig_table_at(blob.data()), recs, &off);
	if (total < 0) return total;
	std::vector<size_t> cut;
	bam_cuts(off, cut);
	if ((cut.size() - 1) * BGZF_MAX > cap) return 0;
	return (int64_t)bgzf_blocks_at(recs.data(), cut, level, out);
}
