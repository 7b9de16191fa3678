// tests/sai_sort_main.cpp -- host check of salt_amd/csrc/salt_sai_sort.h (built and run by tests/test_sai_sort_model.py).
// Three runs of the seed-interval sort on the same list must leave the same order of (sp, ep, off) triples:
//   1. the serial replica the heavy kernels ran before the header existed (three arrays addressed by index, compares on
//      whole triples), kept below as the independently written form: it is the one the GPU suite held to the oracle;
//   2. the header's template on the triples in place (what the device runs on a long list, one lane over LDS);
//   3. the header's template on a key and an index per element plus a packed stack word per entry (what the device
//      runs on a list of up to 64 seeds held in lanes), the triples moved afterwards by the permutation.
// Forms 2 and 3 share the template, so only form 1 stands against an error in the template itself.  Form 3 models the
// device's SaiLaneSort (salt_align.hip) and does not run it: the readlanes, the lane selects and the 8/8/16-bit stack word
// are repeated here by hand, and an error in the device struct's own code shows only in the GPU parity tests.
// Lists: every length 0 .. 64 (and longer ones for forms 1 and 2), keys drawn from 1, 2, 3, 4, 8, 17 and many distinct
// values so that runs of equal keys meet the partition pass and the insertion pass, sorted / reversed / all-equal lists.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../salt_amd/csrc/salt_sai_sort.h"

struct Tri { uint32_t sp, ep, off; };
static inline bool tri_lt(const Tri &a, const Tri &b) { return a.ep - a.sp < b.ep - b.sp; }

// ---- form 1: the project's earlier replica, as the heavy kernels ran it before the template: the triples in three arrays,
// addressed by index, every compare on whole triples, the postponed ranges in three plain arrays.  Kept here word for word
// (less the list selector and the device attributes) as the form that was written and checked against the oracle on its own.
struct Sai { uint32_t sp, ep, off; };
struct SaiArrays { uint32_t *sp, *ep, *off; };
static inline Sai old_get(const SaiArrays &s, int i) { return Sai{ s.sp[i], s.ep[i], s.off[i] }; }
static inline void old_set(SaiArrays &s, int i, Sai v) { s.sp[i] = v.sp; s.ep[i] = v.ep; s.off[i] = v.off; }
static inline bool old_ltv(Sai a, Sai b) { return a.ep - a.sp < b.ep - b.sp; }
static inline bool old_lt(const SaiArrays &s, int i, int j) { return old_ltv(old_get(s, i), old_get(s, j)); }
static inline void old_swap(SaiArrays &s, int i, int j) { Sai a = old_get(s, i), b = old_get(s, j); old_set(s, i, b); old_set(s, j, a); }

static void old_insertsort(SaiArrays &s, int lo, int hi)
{
    for (int i = lo + 1; i < hi; ++i)
        for (int j = i; j > lo && old_lt(s, j, j - 1); --j) old_swap(s, j, j - 1);
}

static void old_combsort(SaiArrays &s, int base, int n)
{
    const double shrink = 1.2473309501039786540366528676643;
    int gap = n; bool do_swap;
    do {
        if (gap > 2) { gap = (int)(gap / shrink); if (gap == 9 || gap == 10) gap = 11; }
        do_swap = false;
        for (int i = 0; i < n - gap; ++i)
            if (old_lt(s, base + i + gap, base + i)) { old_swap(s, base + i, base + i + gap); do_swap = true; }
    } while (do_swap || gap > 2);
    if (gap != 1) old_insertsort(s, base, base + n);
}

static void old_introsort(SaiArrays &s, int n)
{
    if (n < 1) return;
    if (n == 2) { if (old_lt(s, 1, 0)) old_swap(s, 0, 1); return; }
    int d; for (d = 2; (1 << d) < n; ++d) { }
    d <<= 1;
    int st_l[24], st_r[24], st_d[24], top = 0;
    int lo = 0, hi = n - 1;
    for (;;) {
        if (lo < hi) {
            if (--d == 0) { old_combsort(s, lo, hi - lo + 1); hi = lo; continue; }
            int i = lo, j = hi, k = i + ((j - i) >> 1) + 1;
            if (old_lt(s, k, i)) { if (old_lt(s, k, j)) k = j; }
            else k = old_lt(s, j, i) ? i : j;
            Sai rp = old_get(s, k);
            if (k != hi) old_swap(s, k, hi);
            for (;;) {
                do ++i; while (old_ltv(old_get(s, i), rp));
                do --j; while (i <= j && old_ltv(rp, old_get(s, j)));
                if (j <= i) break;
                old_swap(s, i, j);
            }
            old_swap(s, i, hi);
            if (i - lo > hi - i) {
                if (i - lo > 16 && top < 24) { st_l[top] = lo; st_r[top] = i - 1; st_d[top] = d; ++top; }
                lo = hi - i > 16 ? i + 1 : hi;
            } else {
                if (hi - i > 16 && top < 24) { st_l[top] = i + 1; st_r[top] = hi; st_d[top] = d; ++top; }
                hi = i - lo > 16 ? i - 1 : lo;
            }
        } else {
            if (top == 0) { old_insertsort(s, 0, n); return; }
            --top; lo = st_l[top]; hi = st_r[top]; d = st_d[top];
        }
    }
}

// ---- form 2: the triples in place ----
struct InPlace {
    Tri *a; int st[salt::SAI_STACK][3];
    uint32_t key(int i) const { return a[i].ep - a[i].sp; }
    void swap(int i, int j) { Tri t = a[i]; a[i] = a[j]; a[j] = t; }
    void push(int top, int lo, int hi, int d) { st[top][0] = lo; st[top][1] = hi; st[top][2] = d; }
    void pop(int top, int &lo, int &hi, int &d) const { lo = st[top][0]; hi = st[top][1]; d = st[top][2]; }
};

// ---- form 3: a key, an index and a stack word per lane, as SaiLaneSort (salt_align.hip) keeps them ----
struct Lanes {
    uint32_t k[64], ix[64], stk[64];
    uint32_t key(int i) const { if (i < 0 || i > 63) { std::printf("lane %d read\n", i); std::exit(2); } return k[i]; }
    void swap(int i, int j)
    {
        const uint32_t ki = key(i), kj = key(j), xi = ix[i], xj = ix[j];
        for (int lane = 0; lane < 64; ++lane) {
            if (lane == i) { k[lane] = kj; ix[lane] = xj; }
            if (lane == j) { k[lane] = ki; ix[lane] = xi; }
        }
    }
    void push(int top, int lo, int hi, int d) { stk[top] = (uint32_t)lo | ((uint32_t)hi << 8) | ((uint32_t)d << 16); }
    void pop(int top, int &lo, int &hi, int &d) const { const uint32_t v = stk[top]; lo = (int)(v & 255u); hi = (int)((v >> 8) & 255u); d = (int)(v >> 16); }
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 24); }

static long n_lists = 0;
static int check(const std::vector<Tri> &in)
{
    const int n = (int)in.size();
    std::vector<Tri> a = in, b = in, c = in;
    {
        std::vector<uint32_t> sp((size_t)n), ep((size_t)n), off((size_t)n);
        for (int e = 0; e < n; ++e) { sp[(size_t)e] = in[(size_t)e].sp; ep[(size_t)e] = in[(size_t)e].ep; off[(size_t)e] = in[(size_t)e].off; }
        SaiArrays s{ sp.data(), ep.data(), off.data() };
        old_introsort(s, n);
        for (int e = 0; e < n; ++e) a[(size_t)e] = Tri{ sp[(size_t)e], ep[(size_t)e], off[(size_t)e] };
    }
    InPlace ip; ip.a = b.data();
    salt::sai_introsort(ip, n);
    if (n <= 64 && n >= 2) {
        Lanes l;
        for (int e = 0; e < 64; ++e) { l.k[e] = e < n ? in[e].ep - in[e].sp : 0u; l.ix[e] = (uint32_t)e; l.stk[e] = 0; }
        salt::sai_introsort(l, n);
        for (int e = 0; e < n; ++e) c[e] = in[l.ix[e]];
    } else c = b;
    ++n_lists;
    for (int e = 0; e < n; ++e) {
        const bool same2 = a[e].sp == b[e].sp && a[e].ep == b[e].ep && a[e].off == b[e].off;
        const bool same3 = a[e].sp == c[e].sp && a[e].ep == c[e].ep && a[e].off == c[e].off;
        if (!same2 || !same3) { std::printf("list of %d: place %d differs (in place %d, lanes %d)\n", n, e, (int)same2, (int)same3); return 1; }
        if (e && tri_lt(a[e], a[e - 1])) { std::printf("list of %d: not sorted at %d\n", n, e); return 1; }
    }
    return 0;
}

int main()
{
    static const uint32_t n_keys[] = { 1, 2, 3, 4, 8, 17, 1000000 };
    int bad = 0;
    for (int n = 0; n <= 200 && !bad; n = n < 70 ? n + 1 : n + 13)
        for (uint32_t nk : n_keys)
            for (int rep = 0; rep < (n <= 64 ? 40 : 6) && !bad; ++rep) {
                std::vector<Tri> v((size_t)n);
                for (int e = 0; e < n; ++e) {
                    const uint32_t sp = rnd() % 1000000u, key = rnd() % nk;
                    v[(size_t)e] = Tri{ sp, sp + key, (uint32_t)e };       // off = where it stood: tells equal keys apart
                }
                if (rep == 1) for (int e = 0; e < n; ++e) v[(size_t)e].ep = v[(size_t)e].sp + (uint32_t)e;             // sorted
                if (rep == 2) for (int e = 0; e < n; ++e) v[(size_t)e].ep = v[(size_t)e].sp + (uint32_t)(n - e);       // reversed
                if (rep == 3) for (int e = 0; e < n; ++e) v[(size_t)e].ep = v[(size_t)e].sp + (uint32_t)(e / 17);      // runs of 17 equal keys
                if (rep == 4) for (int e = 0; e < n; ++e) v[(size_t)e].ep = v[(size_t)e].sp + (uint32_t)((n - e) / 8); // runs of 8, descending
                bad |= check(v);
            }
    std::printf("%ld lists, %s\n", n_lists, bad ? "FAILED" : "all three forms agree");
    return bad;
}
