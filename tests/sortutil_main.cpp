// sortutil_main.cpp — stand-alone driver of mpibwa_amd/csrc/sortutil.h for tests/test_sortutil.py (built with ASan + UBSan).
// stdin: one key list per line ("n k0 k1 ... k(n-1)").  Per list it sorts an order array under "key less" and prints
//   F <order>   ks_introsort_at, frame arrays of exactly 16 (n <= 512) or 32 (n <= 4096) ints each: the device capacities, so that a
//               frame beyond the stated bound is an out-of-bounds write the sanitizer reports
//   S <order>   ks_small_introsort_at, for n <= 16
//   H <order>   the host's ks_introsort over a T* (the keys with their element numbers)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sortutil.h"

struct Elem { long key; int idx; };

static void print(char tag, const std::vector<unsigned short> &o)
{
	std::printf("%c", tag);
	for (unsigned short v : o) std::printf(" %d", (int)v);
	std::printf("\n");
}

int main()
{
	int n;
	while (std::scanf("%d", &n) == 1) {
		if (n < 0 || n > 4096) return 2;
		std::vector<long> key(n);
		for (int i = 0; i < n; ++i)
			if (std::scanf("%ld", &key[i]) != 1) return 2;
		auto lt = [&](int x, int y) { return key[x] < key[y]; };
		std::vector<unsigned short> o(n);
		auto at = [&](int k) -> unsigned short & { return o[k]; };
		for (int i = 0; i < n; ++i) o[i] = (unsigned short)i;
		{
			const int frames = n <= 512 ? 16 : 32;
			int *fs = (int *)std::malloc(frames * sizeof(int)), *ft = (int *)std::malloc(frames * sizeof(int)), *fd = (int *)std::malloc(frames * sizeof(int));
			mbw::ks_introsort_at(n, at, mbw::KsFramesAt{fs, ft, fd}, lt);
			std::free(fs); std::free(ft); std::free(fd);
		}
		print('F', o);
		if (n <= 16) {
			for (int i = 0; i < n; ++i) o[i] = (unsigned short)i;
			mbw::ks_small_introsort_at(n, at, lt);
			print('S', o);
		}
		std::vector<Elem> e(n);
		for (int i = 0; i < n; ++i) e[i] = Elem{key[i], i};
		mbw::ks_introsort((size_t)n, e.data(), [](const Elem &x, const Elem &y) { return x.key < y.key; });
		for (int i = 0; i < n; ++i) o[i] = (unsigned short)e[i].idx;
		print('H', o);
	}
	return 0;
}
