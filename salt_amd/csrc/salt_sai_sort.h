// salt_amd/csrc/salt_sai_sort.h -- klib's introsort (ksort.h:159-228) as the reference runs it on a read's seed intervals
// (alnse.c:307-308, order: interval size ep - sp, alnse.c:35), written once over an accessor so that the same steps run
//   - on the (sp, ep, off) triples in LDS, one lane per list (lists of more than 64 seeds: the big shapes),
//   - on a key and an index per element held one element a lane (k_heavy's usual shape), every step wave-uniform,
//   - on plain arrays on the host (tests/sai_sort_main.cpp).
// The sort is not stable and the order of equal keys decides which rows lie in front of the locate cap, so every accessor
// must see the same compares and swaps: the only things the algorithm asks of one are
//   uint32_t key(int i)                      the key of element i
//   void     swap(int i, int j)              exchange elements i and j
//   void     push(int top, int lo, int hi, int d) / void pop(int top, int &lo, int &hi, int &d)    the stack of postponed ranges
// Plain C++: no device construct in here (SAI_FN adds the attributes under hipcc).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SAI_FN __device__ __forceinline__
#else
#define SAI_FN inline
#endif

namespace salt {

static constexpr int SAI_STACK = 24;         // postponed ranges (more are dropped to the final insertion pass, as before)

template <class A> SAI_FN void sai_insertsort(A &a, int lo, int hi)
{
    for (int i = lo + 1; i < hi; ++i)
        for (int j = i; j > lo && a.key(j) < a.key(j - 1); --j) a.swap(j, j - 1);
}

template <class A> SAI_FN void sai_combsort(A &a, int base, int n)
{
    const double shrink = 1.2473309501039786540366528676643;
    int gap = n; bool do_swap;
    do {
        if (gap > 2) { gap = (int)(gap / shrink); if (gap == 9 || gap == 10) gap = 11; }
        do_swap = false;
        for (int i = 0; i < n - gap; ++i)
            if (a.key(base + i + gap) < a.key(base + i)) { a.swap(base + i, base + i + gap); do_swap = true; }
    } while (do_swap || gap > 2);
    if (gap != 1) sai_insertsort(a, base, base + n);
}

template <class A> SAI_FN void sai_introsort(A &a, int n)
{
    if (n < 1) return;
    if (n == 2) { if (a.key(1) < a.key(0)) a.swap(0, 1); return; }
    int d; for (d = 2; (1 << d) < n; ++d) { }
    d <<= 1;
    int top = 0;
    int lo = 0, hi = n - 1;
    for (;;) {
        if (lo < hi) {
            if (--d == 0) { sai_combsort(a, lo, hi - lo + 1); hi = lo; continue; }
            int i = lo, j = hi, k = i + ((j - i) >> 1) + 1;
            if (a.key(k) < a.key(i)) { if (a.key(k) < a.key(j)) k = j; }
            else k = a.key(j) < a.key(i) ? i : j;
            const uint32_t rp = a.key(k);
            if (k != hi) a.swap(k, hi);
            for (;;) {
                do ++i; while (a.key(i) < rp);
                do --j; while (i <= j && rp < a.key(j));
                if (j <= i) break;
                a.swap(i, j);
            }
            a.swap(i, hi);
            if (i - lo > hi - i) {
                if (i - lo > 16 && top < SAI_STACK) { a.push(top, lo, i - 1, d); ++top; }
                lo = hi - i > 16 ? i + 1 : hi;
            } else {
                if (hi - i > 16 && top < SAI_STACK) { a.push(top, i + 1, hi, d); ++top; }
                hi = i - lo > 16 ? i - 1 : lo;
            }
        } else {
            if (top == 0) { sai_insertsort(a, 0, n); return; }
            --top; a.pop(top, lo, hi, d);
        }
    }
}

}  // namespace salt
