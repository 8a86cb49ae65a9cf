// chainmath_main.cpp — stand-alone driver of mpibwa_amd/csrc/chainmath.h for tests/test_chainmath.py (built with ASan + UBSan).
// stdin: one case per line, a letter and its integers (a float comes as its 32 bits); stdout: one line of results per case.
//   C off0 off1 ...                                         sets the contig table (where every contig starts): n_seqs
//   T g0 g1 ...                                             sets the gap table (cal_max_gap of 0, 1, ... query bases): its length
//   R l_pac pos                                             depos(pos), pos2rid of it
//   I l_pac rb re                                           intv2rid
//   S l_pac off len is_rev                                  strand_span: beg, end
//   M l_pac w max_chain_gap first_r first_q last_r last_q last_len rb qb len      merge_verdict
//   W (rbeg qbeg len)*                                      CoverSum over the query, over the reference, chain_weight_of
//   O mask_level max_chain_gap bj ej alt_j bi ei alt_i      flt_large_overlap
//   D drop_ratio min_seed_len wj wi                         flt_drops
//   X max_chain_extend kept0 kept1 ...                      flt_cut_extend: the flags afterwards
//   E lq rbeg qbeg len                                      seed_reach: b, e
//   N l_pac lo hi first_r far_beg far_end                   chain_window: rmax0, rmax1
//   H l_pac lq rid (rbeg qbeg len)*                         a chain as the callers put the pieces together: far_beg, far_end, rmax0, rmax1
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>
#include "chainmath.h"

using namespace mbw;

static float as_float(long long bits)
{
	const uint32_t u = (uint32_t)bits;
	float f;
	std::memcpy(&f, &u, sizeof f);
	return f;
}

int main()
{
	std::vector<int64_t> contigs;
	std::vector<int> gaps;
	std::string line;
	while (std::getline(std::cin, line)) {
		if (line.empty()) continue;
		const char c = line[0];
		std::vector<long long> v;
		const char *p = line.c_str() + 1;
		for (;;) {
			char *end;
			const long long x = std::strtoll(p, &end, 0);
			if (end == p) break;
			v.push_back(x);
			p = end;
		}
		const size_t n = v.size();
		auto off = [&contigs](int i) -> int64_t { return contigs.at(i); };
		auto gap = [&gaps](int q) -> int { return gaps.at(q); };
		const int n_seqs = (int)contigs.size();
		if (c == 'C') {
			contigs.assign(v.begin(), v.end());
			std::printf("%zu\n", contigs.size());
		} else if (c == 'T') {
			gaps.assign(v.begin(), v.end());
			std::printf("%zu\n", gaps.size());
		} else if (c == 'R' && n == 2) {
			const int64_t f = depos(v[0], v[1]);
			std::printf("%" PRId64 " %d\n", f, pos2rid(off, n_seqs, v[0], f));
		} else if (c == 'I' && n == 3) std::printf("%d\n", intv2rid(off, n_seqs, v[0], v[1], v[2]));
		else if (c == 'S' && n == 4) {
			int64_t b, e;
			strand_span(v[0], v[1], v[2], v[3] != 0, &b, &e);
			std::printf("%" PRId64 " %" PRId64 "\n", b, e);
		} else if (c == 'M' && n == 11)
			std::printf("%d\n", merge_verdict(v[0], (int)v[1], (int)v[2], v[3], (int)v[4], v[5], (int)v[6], (int)v[7], v[8], (int)v[9], (int)v[10]));
		else if (c == 'W' && n % 3 == 0) {
			CoverSum on_query, on_ref;
			for (size_t k = 0; k < n; k += 3) on_query.add(v[k + 1], (int)v[k + 2]);
			for (size_t k = 0; k < n; k += 3) on_ref.add(v[k], (int)v[k + 2]);
			std::printf("%d %d %d\n", on_query.w, on_ref.w, chain_weight_of(on_query.w, on_ref.w));
		} else if (c == 'O' && n == 8)
			std::printf("%d\n", (int)flt_large_overlap(as_float(v[0]), (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], (int)v[7]));
		else if (c == 'D' && n == 4) std::printf("%d\n", (int)flt_drops(as_float(v[0]), (int)v[1], (int)v[2], (int)v[3]));
		else if (c == 'X' && n >= 1) {
			std::vector<int> kept(v.begin() + 1, v.end());
			flt_cut_extend((int)kept.size(), [&kept](int i) -> int & { return kept.at(i); }, (int)v[0]);
			for (size_t k = 0; k < kept.size(); ++k) std::printf("%s%d", k ? " " : "", kept[k]);
			std::printf("\n");
		} else if (c == 'E' && n == 4) {
			int64_t b, e;
			seed_reach(v[1], (int)v[2], (int)v[3], (int)v[0], gap, &b, &e);
			std::printf("%" PRId64 " %" PRId64 "\n", b, e);
		} else if (c == 'N' && n == 6) {
			int64_t r0, r1;
			chain_window(v[0], v[1], v[2], v[3], v[4], v[5], &r0, &r1);
			std::printf("%" PRId64 " %" PRId64 "\n", r0, r1);
		} else if (c == 'H' && n >= 6 && n % 3 == 0) {
			const int64_t l_pac = v[0], first_r = v[3];
			const int lq = (int)v[1], rid = (int)v[2];
			// (the contig's length as the kernels have it: up to the next contig's start, l_pac behind the last one)
			const int64_t len = (rid + 1 < n_seqs ? off(rid + 1) : l_pac) - off(rid);
			int64_t fb, fe, lo = l_pac << 1, hi = 0, r0, r1;
			strand_span(l_pac, off(rid), len, first_r >= l_pac, &fb, &fe);
			for (size_t k = 3; k < n; k += 3) {
				int64_t b, e;
				seed_reach(v[k], (int)v[k + 1], (int)v[k + 2], lq, gap, &b, &e);
				lo = b < lo ? b : lo;
				hi = e > hi ? e : hi;
			}
			chain_window(l_pac, lo, hi, first_r, fb, fe, &r0, &r1);
			std::printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", fb, fe, r0, r1);
		} else return 2;
	}
	return 0;
}
