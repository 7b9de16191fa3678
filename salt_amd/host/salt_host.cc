// salt_amd/host/salt_host.cc -- host side of the drop-in: index files in, SAM text out.
// See include/salt_host.h for the reference interfaces each entry point mirrors.
#include "../../include/salt_host.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdarg>
#include <cmath>
#include <fstream>
#include <map>
#include <mutex>
#include <sstream>
#include <algorithm>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;

struct Ann { int64_t offset; int32_t len; int32_t n_ambs; std::string name; };
struct Amb { int64_t offset; int32_t len; char amb; };

bool read_file(const std::string &fn, std::vector<uint8_t> &out)
{
    std::ifstream f(fn, std::ios::binary | std::ios::ate);
    if (!f) { g_err = "cannot open " + fn; return false; }
    std::streamsize n = f.tellg();
    f.seekg(0);
    out.resize((size_t)n);
    if (n && !f.read(reinterpret_cast<char *>(out.data()), n)) { g_err = "short read on " + fn; return false; }
    return true;
}

inline uint32_t u32_at(const std::vector<uint8_t> &b, size_t word) { uint32_t v; memcpy(&v, b.data() + 4 * word, 4); return v; }

} // namespace

struct salt_index {
    std::vector<uint32_t> c_bwt, c_sa, lkt, r_bwt, r_occ, r_major, r_sa, ref;
    std::vector<uint8_t> pac;
    std::vector<Ann> anns;
    std::vector<Amb> ambs;
    int64_t l_pac = 0;
    int32_t seed_len = 0;
    salt_host_index_t view;
    mutable std::vector<uint32_t> snp_pos; mutable std::once_flag snp_once;      // the SNP sites' genome positions, listed by the first salt_snp_* call
};

extern "C" const char *salt_host_last_error(void) { return g_err.c_str(); }

extern "C" void salt_lkt_build(const uint8_t *pac, uint32_t l_ref, int len, uint32_t *item)
{
    // counts of every 12-mer start + the `len` A-padded tail suffixes, then prefix sums
    // (Index_src/LookUpTable.c:70-150; the padded tail is why a bucket may hold a too-short suffix)
    const uint32_t n_item = (1u << (2 * len)) + 1, mask = n_item - 2;
    memset(item, 0, (size_t)n_item * 4);
    uint32_t x = 0;
    for (uint32_t i = 0; i < l_ref; ++i) {
        x = ((x << 2) & mask) | ((pac[i >> 2] >> ((~i & 3u) << 1)) & 3u);
        if (i + 1 >= (uint32_t)len) ++item[x + 1];
    }
    for (int i = 0; i < len; ++i) { x = (x << 2) & mask; ++item[x + 1]; }
    for (uint32_t i = 1; i < n_item; ++i) item[i] += item[i - 1];
}

extern "C" salt_index_t *salt_index_load(const char *prefix_c, int rebuild_lkt)
{
    const std::string p(prefix_c);
    std::vector<uint8_t> b;
    salt_index *ix = new salt_index();
    salt_host_index_t &v = ix->view;
    memset(&v, 0, sizeof v);
    auto bail = [&](const std::string &m) -> salt_index_t * { if (!m.empty()) g_err = m; delete ix; return nullptr; };

    if (!read_file(p + ".R.seedLen", b) || b.size() < 4) return bail(b.size() < 4 ? "seed length can't be parsed: " + p + ".R.seedLen" : "");
    memcpy(&ix->seed_len, b.data(), 4);

    if (!read_file(p + ".C.bwt", b)) return bail("");
    if (b.size() < 20 || b.size() % 4) return bail(p + ".C.bwt: malformed");
    v.c_primary = u32_at(b, 0);
    for (int i = 0; i < 4; ++i) v.c_L2[i + 1] = u32_at(b, 1 + i);
    v.c_seq_len = v.c_L2[4];
    ix->c_bwt.assign(reinterpret_cast<const uint32_t *>(b.data()) + 5, reinterpret_cast<const uint32_t *>(b.data() + b.size()));
    v.c_bwt_size = (uint32_t)ix->c_bwt.size();

    if (!read_file(p + ".C.sa", b)) return bail("");
    if (b.size() < 28) return bail(p + ".C.sa: malformed");
    if (u32_at(b, 0) != v.c_primary || u32_at(b, 6) != v.c_seq_len) return bail("SA-BWT inconsistency: " + p + ".C.sa");
    v.c_sa_intv = u32_at(b, 5);
    if (v.c_sa_intv == 0) return bail(p + ".C.sa: zero sampling interval");
    v.c_n_sa = (v.c_seq_len + v.c_sa_intv) / v.c_sa_intv;
    if (b.size() < 28 + 4 * (size_t)(v.c_n_sa - 1)) return bail(p + ".C.sa: truncated");
    ix->c_sa.resize(v.c_n_sa);
    ix->c_sa[0] = 0xFFFFFFFFu;
    memcpy(ix->c_sa.data() + 1, b.data() + 28, 4 * (size_t)(v.c_n_sa - 1));

    if (!read_file(p + ".R.backward.bwt", b)) return bail("");
    if (b.size() < 32) return bail(p + ".R.backward.bwt: malformed");
    v.r_text_len = u32_at(b, 0); v.r_inv_sa0 = u32_at(b, 1);
    for (int i = 0; i < 5; ++i) v.r_cum[i + 1] = u32_at(b, 2 + i);
    v.r_bwt_words = u32_at(b, 7);
    if (b.size() < 32 + 4 * (size_t)v.r_bwt_words) return bail(p + ".R.backward.bwt: truncated");
    ix->r_bwt.assign((size_t)v.r_bwt_words + 64, 0);
    memcpy(ix->r_bwt.data(), b.data() + 32, 4 * (size_t)v.r_bwt_words);

    if (!read_file(p + ".R.backward.occ", b)) return bail("");
    {
        if (b.size() < 8) return bail(p + ".R.backward.occ: malformed");
        uint32_t n = u32_at(b, 0);
        if (b.size() < 8 + 4 * (size_t)n) return bail(p + ".R.backward.occ: truncated");
        ix->r_occ.assign(reinterpret_cast<const uint32_t *>(b.data()) + 1, reinterpret_cast<const uint32_t *>(b.data()) + 1 + n);
        uint32_t m = u32_at(b, 1 + n);
        if (b.size() < 8 + 4 * ((size_t)n + m)) return bail(p + ".R.backward.occ: truncated");
        ix->r_major.assign(reinterpret_cast<const uint32_t *>(b.data()) + 2 + n, reinterpret_cast<const uint32_t *>(b.data()) + 2 + n + m);
        v.r_occ_words = n; v.r_major_words = m;
    }
    if (!read_file(p + ".R.backward.sa", b)) return bail("");
    {
        if (b.size() < 4) return bail(p + ".R.backward.sa: malformed");
        uint32_t n = u32_at(b, 0);
        if (b.size() < 4 + 4 * (size_t)n) return bail(p + ".R.backward.sa: truncated");
        ix->r_sa.assign(reinterpret_cast<const uint32_t *>(b.data()) + 1, reinterpret_cast<const uint32_t *>(b.data()) + 1 + n);
        v.r_n_sa = n;
    }
    if (!read_file(p + ".ref", b)) return bail("");
    {
        if (b.size() < 4) return bail(p + ".ref: malformed");
        v.ref_len = u32_at(b, 0);
        size_t nw = ((size_t)v.ref_len + 7) / 8;
        if (b.size() < 4 + 4 * nw) return bail(p + ".ref: truncated");
        ix->ref.assign(nw + 4, 0);
        memcpy(ix->ref.data(), b.data() + 4, 4 * nw);
    }
    {   // .C.ann / .C.amb (text, BWA 0.5/0.6 layout)
        std::ifstream f(p + ".C.ann");
        if (!f) return bail("cannot open " + p + ".C.ann");
        long long lp; int n_seqs; unsigned seed;
        if (!(f >> lp >> n_seqs >> seed)) return bail(p + ".C.ann: malformed");
        ix->l_pac = lp;
        for (int i = 0; i < n_seqs; ++i) {
            unsigned gi; Ann a; std::string rest; long long off;
            if (!(f >> gi >> a.name)) return bail(p + ".C.ann: malformed");
            std::getline(f, rest);
            if (!(f >> off >> a.len >> a.n_ambs)) return bail(p + ".C.ann: malformed");
            a.offset = off;
            ix->anns.push_back(a);
        }
        std::ifstream g(p + ".C.amb");
        if (!g) return bail("cannot open " + p + ".C.amb");
        long long lp2; int ns2, n_holes;
        if (!(g >> lp2 >> ns2 >> n_holes)) return bail(p + ".C.amb: malformed");
        if (lp2 != lp || ns2 != n_seqs) return bail("inconsistent .ann and .amb files");
        for (int i = 0; i < n_holes; ++i) {
            long long off; Amb a; std::string s;
            if (!(g >> off >> a.len >> s)) return bail(p + ".C.amb: malformed");
            a.offset = off; a.amb = s.empty() ? 'N' : s[0];
            ix->ambs.push_back(a);
        }
    }
    if (!read_file(p + ".C.pac", ix->pac)) return bail("");
    if (ix->pac.size() < (size_t)ix->l_pac / 4 + 1) return bail(p + ".C.pac: truncated");
    ix->pac.resize((size_t)ix->l_pac / 4 + 8, 0);
    {
        std::ifstream f(p + ".C.lkt", std::ios::binary);
        if (f) {
            int32_t len = 0;
            f.read(reinterpret_cast<char *>(&len), 4);
            if (!f || len < 1 || len > 14) return bail(p + ".C.lkt: malformed");
            v.lkt_len = (uint32_t)len; v.lkt_n = (1u << (2 * len)) + 1;
            ix->lkt.resize(v.lkt_n);
            f.read(reinterpret_cast<char *>(ix->lkt.data()), 4 * (std::streamsize)v.lkt_n);
            if (!f) return bail(p + ".C.lkt: truncated");
        } else if (rebuild_lkt) {
            v.lkt_len = 12; v.lkt_n = (1u << 24) + 1;
            ix->lkt.resize(v.lkt_n);
            salt_lkt_build(ix->pac.data(), (uint32_t)ix->l_pac, 12, ix->lkt.data());
        } else return bail("cannot open " + p + ".C.lkt");
    }
    v.c_bwt = ix->c_bwt.data(); v.c_sa = ix->c_sa.data(); v.lkt = ix->lkt.data();
    v.r_bwt = ix->r_bwt.data(); v.r_occ = ix->r_occ.data(); v.r_major = ix->r_major.data(); v.r_sa = ix->r_sa.data();
    v.ref = ix->ref.data();
    v.l_seed = ix->seed_len;
    return ix;
}

extern "C" void salt_index_free(salt_index_t *ix) { delete ix; }
extern "C" const salt_host_index_t *salt_index_host_view(const salt_index_t *ix) { return &ix->view; }
extern "C" int32_t salt_index_seed_len(const salt_index_t *ix) { return ix->seed_len; }
extern "C" const uint8_t *salt_index_pac(const salt_index_t *ix, uint64_t *l_pac) { if (l_pac) *l_pac = (uint64_t)ix->l_pac; return ix->pac.data(); }
extern "C" int32_t salt_index_n_seqs(const salt_index_t *ix) { return (int32_t)ix->anns.size(); }
extern "C" int salt_index_seq(const salt_index_t *ix, int32_t i, int64_t *offset, int32_t *len, const char **name)
{
    if (!ix || i < 0 || (size_t)i >= ix->anns.size()) return -1;
    if (offset) *offset = ix->anns[(size_t)i].offset;
    if (len) *len = ix->anns[(size_t)i].len;
    if (name) *name = ix->anns[(size_t)i].name.c_str();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// SAM text
// ---------------------------------------------------------------------------------------------
namespace {

struct Out {
    char *s; size_t n, cap; bool ovf;
    void put(char c) { if (n + 1 < cap) s[n++] = c; else ovf = true; }
    void puts(const char *t) { while (*t) put(*t++); }
    void putu(uint64_t v) { char tmp[24]; int k = 0; do { tmp[k++] = (char)('0' + v % 10); v /= 10; } while (v); while (k) put(tmp[--k]); }
    int done() { if (ovf || n >= cap) return -1; s[n] = 0; return (int)n; }
};

int seq_id(const salt_index *ix, int64_t coor)          // bns_coor_pac2real's sequence search (bntseq.c:269-289)
{
    int left = 0, mid = 0, right = (int)ix->anns.size();
    while (left < right) {
        mid = (left + right) >> 1;
        if (coor >= ix->anns[mid].offset) {
            if (mid == (int)ix->anns.size() - 1) break;
            if (coor < ix->anns[mid + 1].offset) break;
            left = mid + 1;
        } else right = mid;
    }
    return mid;
}

inline uint32_t pac_at(const salt_index *ix, uint32_t l) { return (ix->pac[l >> 2] >> ((~l & 3u) << 1)) & 3u; }
inline uint32_t mask_at(const salt_index *ix, uint32_t l) { return (ix->ref[l >> 3] >> (4 * (l & 7u))) & 15u; }

void put_cigar(Out &o, const uint16_t *ops, int n)
{
    for (int i = 0; i < n; ++i) { o.putu(ops[i] >> 4); o.put("MID?"[ops[i] & 3]); }
}

void put_xa(Out &o, const salt_index *ix, const salt_sam_opt_t *opt, int L, const salt_result_t *q)
{
    // XA (sam.c:186-240)
    bool first = true; int h = 0;
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < q->n_hits[s]; ++i, ++h) {
            const salt_hit_t &hit = q->hits[s][i];
            if (hit.pos == q->pos) continue;
            if (first) { o.puts("\tXA:Z:"); first = false; }
            int r2 = seq_id(ix, hit.pos);
            o.puts(ix->anns[r2].name.c_str()); o.put(','); o.put("+-"[s]);
            o.putu((uint64_t)((int64_t)hit.pos - ix->anns[r2].offset + 1)); o.put(',');
            if (opt->print_xa_cigar) {
                if (hit.is_gap) put_cigar(o, q->hit_cigar[h], q->hit_n_cigar[h]);
                else { o.putu((uint64_t)L); o.put('M'); }
                o.put(',');
            } else o.puts("*,");
            o.putu(hit.n_diff); o.put(';');
        }
}

void put_md_nm(Out &o, const salt_index *ix, const uint8_t *sq, const salt_result_t *q)
{
    static const char NT[] = "ACGTN";
    // MD / NM / XV against the 2-bit pac (sam.c:246-328)
    {
        int nm = 0, n_match = 0, n_rs = 0, rsv[64];
        uint32_t rp = q->pos; int si = q->seq_start;
        o.puts("\tMD:Z:");
        for (int c = 0; c < q->n_cigar; ++c) {
            int n = q->cigar[c] >> 4, op = q->cigar[c] & 15;
            if (op == 0) {
                for (int i = 0; i < n; ++i, ++rp, ++si) {
                    uint32_t bt = pac_at(ix, rp);
                    if (bt == sq[si]) { ++n_match; continue; }
                    if (sq[si] < 5 && (mask_at(ix, rp) & (1u << sq[si])) != 0 && n_rs < 64) rsv[n_rs++] = si - q->seq_start;
                    ++nm;
                    if (n_match) o.putu((uint64_t)n_match);
                    n_match = 0;
                    o.put(NT[bt]);
                }
            } else if (op == 1) { nm += n; si += n; }
            else if (op == 2) {
                if (n_match) o.putu((uint64_t)n_match);
                n_match = 0; nm += n; o.put('^');
                for (int i = 0; i < n; ++i, ++rp) o.put(NT[pac_at(ix, rp)]);
            }
        }
        if (n_match) o.putu((uint64_t)n_match);
        o.puts("\tNM:i:"); o.putu((uint64_t)nm);
        if (n_rs > 0) { o.puts("\tXV:i:"); for (int i = 0; i < n_rs; ++i) { if (i) o.put(','); o.putu((uint64_t)rsv[i]); } }
    }
}

} // namespace

extern "C" int salt_isize_infer(const salt_index_t *ix, uint32_t n_pairs, const uint32_t *offs, const salt_result_t *res,
                                uint32_t *min_tlen, uint32_t *max_tlen, uint32_t *n_used)
{
    std::vector<uint32_t> t;
    for (uint32_t i = 0; i < n_pairs; ++i) {
        const salt_result_t &a = res[2 * (size_t)i], &b = res[2 * (size_t)i + 1];
        if (a.skipped || b.skipped || a.pos == 0xFFFFFFFFu || b.pos == 0xFFFFFFFFu || a.is_gap || b.is_gap) continue;
        if (a.n_hits[0] || a.n_hits[1] || b.n_hits[0] || b.n_hits[1]) continue;
        if (a.strand > 1 || b.strand > 1 || a.strand == b.strand) continue;
        const bool a_fwd = a.strand == 0;
        const salt_result_t &f = a_fwd ? a : b, &r = a_fwd ? b : a;
        const uint32_t len_r = a_fwd ? offs[2 * (size_t)i + 2] - offs[2 * (size_t)i + 1] : offs[2 * (size_t)i + 1] - offs[2 * (size_t)i];
        if (r.pos < f.pos || seq_id(ix, f.pos) != seq_id(ix, r.pos)) continue;
        const uint64_t tl = (uint64_t)r.pos + len_r - f.pos;
        if (tl <= 100000) t.push_back((uint32_t)tl);
    }
    if (n_used) *n_used = (uint32_t)t.size();
    const size_t n = t.size();
    if (n < 25) return -1;
    std::sort(t.begin(), t.end());
    const uint64_t q1 = t[n / 4], q3 = t[3 * n / 4], iqr = q3 - q1;
    const uint64_t lo = q1 > 2 * iqr ? q1 - 2 * iqr : 0, hi = q3 + 2 * iqr;
    uint64_t m = 0, sum = 0;
    for (uint32_t v : t) if (v >= lo && v <= hi) { ++m; sum += v; }
    const uint64_t mean = (sum + m / 2) / m;
    uint64_t var = 0;
    for (uint32_t v : t) if (v >= lo && v <= hi) { const uint64_t d = v > mean ? v - mean : mean - v; var += d * d; }
    var /= m;
    uint64_t sd = 0;
    while ((sd + 1) * (sd + 1) <= var) ++sd;                  // floor(sqrt(var)) ...
    if (sd * sd < var) ++sd;                                  // ... rounded up
    uint64_t wa = mean > 4 * sd ? mean - 4 * sd : 1, wb = mean + 4 * sd;
    wa = std::min<uint64_t>(wa, q1 > 3 * iqr ? q1 - 3 * iqr : 1);
    wb = std::max<uint64_t>(wb, q3 + 3 * iqr);
    *min_tlen = (uint32_t)std::max<uint64_t>(wa, 1); *max_tlen = (uint32_t)wb;
    return 0;
}

extern "C" int salt_cigar_text(const uint16_t *ops, int n_ops, char *buf, size_t cap)
{
    Out o{ buf, 0, cap, false };
    put_cigar(o, ops, n_ops);
    return o.done();
}

extern "C" int salt_sam_header(const salt_index_t *ix, const salt_sam_opt_t *opt, char *buf, size_t cap)
{
    Out o{ buf, 0, cap, false };
    o.puts("@HD\tVN:ec1fec2\tSO:unsorted\n");
    for (const Ann &a : ix->anns) { o.puts("@SQ\tSN:"); o.puts(a.name.c_str()); o.puts("\tLN:"); o.putu((uint64_t)a.len); o.put('\n'); }
    o.puts("@RG\tID:"); o.puts(opt && opt->rg_id ? opt->rg_id : "(null)"); o.put('\n');     // printf("%s", NULL) in sam.c:69
    return o.done();
}

extern "C" int salt_sam_se(const salt_index_t *ix, const salt_sam_opt_t *opt, const char *name, const uint8_t *seq,
                           int32_t L, const char *qual, const salt_result_t *q, char *buf, size_t cap)
{
    Out o{ buf, 0, cap, false };
    if (cap) buf[0] = 0;
    if (q->skipped) return 0;
    static const char NT[] = "ACGTN";
    if (q->pos == 0xFFFFFFFFu) {                                 // sam.c:105-125
        o.puts(name); o.puts("\t4\t*\t0\t0\t*\t*\t0\t0\t");
        for (int i = 0; i < L; ++i) o.put(NT[seq[i] > 4 ? 4 : seq[i]]);
        o.put('\t'); o.puts(qual ? qual : "*");
        return o.done();
    }
    uint8_t rs_stack[1024]; std::vector<uint8_t> rs_heap;       // the reverse complement: no allocation per read for ordinary lengths
    uint8_t *rs = rs_stack;
    if (L > (int)sizeof rs_stack) { rs_heap.resize((size_t)L); rs = rs_heap.data(); }
    if (q->strand) for (int i = 0; i < L; ++i) { uint8_t c = seq[L - 1 - i]; rs[i] = c < 4 ? (uint8_t)(3 - c) : c; }
    const uint8_t *sq = q->strand ? rs : seq;                    // bases as aligned
    int rid = seq_id(ix, q->pos);
    o.puts(name); o.put('\t'); o.putu(q->strand ? 16 : 0); o.put('\t'); o.puts(ix->anns[rid].name.c_str()); o.put('\t');
    o.putu((uint64_t)((int64_t)q->pos - ix->anns[rid].offset + 1)); o.put('\t'); o.putu(q->mapq); o.put('\t');
    put_cigar(o, q->cigar, q->n_cigar);
    o.puts("\t*\t0\t0\t");
    for (int i = 0; i < L; ++i) o.put(NT[sq[i] > 4 ? 4 : sq[i]]);
    o.put('\t');
    if (q->strand) { if (qual) for (int i = L - 1; i >= 0; --i) o.put(qual[i]); else o.put('*'); }
    else o.puts(qual && qual[0] ? qual : "*");
    put_xa(o, ix, opt, L, q);
    if (opt->print_nm_md) put_md_nm(o, ix, sq, q);
    if (opt->rg_id) { o.puts("\tRG:Z:"); o.puts(opt->rg_id); }
    return o.done();
}

// alnpe_sam (sam.c:331-457): both records of pair; each is followed by "\n\n" exactly as the reference's driver
// prints them (the record's own newline plus the printf("%s\n") around it, alnpe.c:640-648)
extern "C" int salt_sam_pe(const salt_index_t *ix, const salt_sam_opt_t *opt, const salt_pe_opt_t *pe, const char *const name[2],
                           const uint8_t *const seq[2], const int32_t l_seq[2], const char *const qual[2],
                           const salt_result_t *q, char *buf, size_t cap)
{
    Out o{ buf, 0, cap, false };
    static const char NT[] = "ACGTN";
    int rid[2] = { -1, -1 }, tlen = 0;
    bool is_map[2] = { false, false };
    uint32_t pos[2] = { 0, 0 };
    for (int i = 0; i < 2; ++i)
        if (q[i].pos != 0xFFFFFFFFu) { is_map[i] = true; rid[i] = seq_id(ix, q[i].pos); pos[i] = q[i].pos - (uint32_t)ix->anns[rid[i]].offset + 1; }
    if (is_map[0] && is_map[1]) {
        if (rid[0] != rid[1]) tlen = 0;
        else if (pos[0] < pos[1]) tlen = (int)(pos[1] + q[1].seq_end - q[1].seq_start + 1 - pos[0]);
        else tlen = (int)(pos[0] + q[0].seq_end - q[1].seq_start + 1 - pos[1]);              // sam.c:355-356: q[1].seq_start in both arms
        if ((uint32_t)tlen > pe->max_tlen || (uint32_t)tlen < pe->min_tlen) tlen = 0;
    }
    for (int i = 0; i < 2; ++i) {
        const int L = l_seq[i];
        uint8_t rs_stack[1024]; std::vector<uint8_t> rs_heap;
        uint8_t *rs = rs_stack;
        if (L > (int)sizeof rs_stack) { rs_heap.resize((size_t)L); rs = rs_heap.data(); }
        for (int k = 0; k < L; ++k) { uint8_t c = seq[i][L - 1 - k]; rs[k] = c < 4 ? (uint8_t)(3 - c) : c; }
        unsigned flag = 0x1;
        if (!is_map[i]) flag |= 0x4;
        if (!is_map[1 - i]) flag |= 0x8;
        if (q[i].strand == 1) flag |= 0x10;
        if (q[1 - i].strand == 1) flag |= 0x20;
        if (tlen != 0) flag |= 0x2;
        flag |= i == 0 ? 0x40 : 0x80;
        o.puts(name[i]); o.put('\t'); o.putu(flag); o.put('\t');
        if (is_map[i]) {
            o.puts(ix->anns[rid[i]].name.c_str()); o.put('\t'); o.putu(pos[i]); o.put('\t'); o.putu(q[i].mapq); o.put('\t');
            if (q[i].seq_start != 0) { o.putu(q[i].seq_start); o.put('S'); }
            put_cigar(o, q[i].cigar, q[i].n_cigar);
            if (q[i].seq_end != (uint32_t)L - 1) { o.putu((uint64_t)(L - (int)q[i].seq_end - 1)); o.put('S'); }
            o.put('\t');
        } else if (is_map[1 - i]) { o.puts(ix->anns[rid[1 - i]].name.c_str()); o.put('\t'); o.putu(pos[1 - i]); o.puts("\t255\t*\t"); }
        else o.puts("*\t0\t255\t*\t");
        if (is_map[1 - i]) {
            if (rid[i] == rid[1 - i] || !is_map[i]) o.puts("=\t"); else { o.puts(ix->anns[rid[1 - i]].name.c_str()); o.put('\t'); }
            o.putu(pos[1 - i]); o.put('\t');
        } else o.puts("*\t0\t");
        if (tlen != 0) { if (q[i].pos >= q[1 - i].pos) o.put('-'); o.putu((uint64_t)tlen); o.put('\t'); }
        else o.puts("0\t");
        const uint8_t *sq = q[i].strand == 1 ? rs : seq[i];
        for (int k = 0; k < L; ++k) o.put(NT[sq[k] > 4 ? 4 : sq[k]]);
        o.put('\t');
        const bool has_q = qual[i] && qual[i][0];
        if (!has_q) o.put('*');
        else if (q[i].strand == 1) for (int k = L - 1; k >= 0; --k) o.put(qual[i][k]);
        else o.puts(qual[i]);
        put_xa(o, ix, opt, L, &q[i]);
        if (opt->print_nm_md && is_map[i]) put_md_nm(o, ix, q[i].strand == 0 ? seq[i] : rs, &q[i]);
        if (opt->rg_id) { o.puts("\tRG:Z:"); o.puts(opt->rg_id); }
        o.puts("\n\n");
    }
    return o.done();
}

// ---------------------------------------------------------------------------------------------
// BAM records (SAM specification 4.2) from SAM lines: the host encoder of `salt --bam`, and the model of the device's
// ---------------------------------------------------------------------------------------------
namespace {

struct Bytes {
    std::vector<uint8_t> b;
    void u8(uint32_t v) { b.push_back((uint8_t)v); }
    void u16(uint32_t v) { u8(v); u8(v >> 8); }
    void u32(uint32_t v) { u16(v); u16(v >> 16); }
    void text(const char *p, const char *e) { b.insert(b.end(), p, e); }
    void set32(size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) b[at + (size_t)i] = (uint8_t)(v >> (8 * i)); }
};

// the specification's bin of the half-open interval [beg, end)
uint32_t reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

bool field_int(const char *p, const char *e, int64_t *v)
{
    if (p == e) return false;
    const bool neg = *p == '-';
    if (neg || *p == '+') ++p;
    if (p == e || e - p > 18) return false;
    int64_t x = 0;
    for (; p < e; ++p) { if (*p < '0' || *p > '9') return false; x = 10 * x + (*p - '0'); }
    *v = neg ? -x : x;
    return true;
}

void bam_int_tag(Bytes &o, int64_t v)
{
    if (v >= 0) {
        if (v <= 0xFF) { o.u8('C'); o.u8((uint32_t)v); }
        else if (v <= 0xFFFF) { o.u8('S'); o.u16((uint32_t)v); }
        else { o.u8('I'); o.u32((uint32_t)v); }
    } else if (v >= -128) { o.u8('c'); o.u8((uint32_t)v); }
    else if (v >= -32768) { o.u8('s'); o.u16((uint32_t)v); }
    else { o.u8('i'); o.u32((uint32_t)v); }
}

struct RefIds {
    std::vector<std::pair<std::string, int32_t>> by_name;       // sorted; the first of equal names wins, as a header's reader would take it
    explicit RefIds(const salt_index *ix)
    {
        for (size_t i = 0; i < ix->anns.size(); ++i) by_name.emplace_back(ix->anns[i].name, (int32_t)i);
        std::stable_sort(by_name.begin(), by_name.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    }
    int32_t find(const char *p, const char *e) const
    {
        const std::string key(p, e);
        auto it = std::lower_bound(by_name.begin(), by_name.end(), key, [](const auto &a, const std::string &k) { return a.first < k; });
        return it != by_name.end() && it->first == key ? it->second : -2;
    }
};

// A SAM record line [l, e) without its newline, split at its tabs: what the BAM encoder and the three host twins below read first.  Every
// refusal is g_err = prefix + why + the line's first 80 bytes, and false.
struct SamLine {
    const char *prefix, *l, *e;
    const char *f[12]; int nf;                                     // starts of the 11 mandatory fields and of the tags
    int64_t flag, pos1, mapq;                                      // set and range-checked by numbers()
    const char *fe(int k) const { return k + 1 < nf ? f[k + 1] - 1 : e; }      // end of field k (the tags: all of them)
    size_t len(int k) const { return (size_t)(fe(k) - f[k]); }
    bool is(int k, char c) const { return len(k) == 1 && *f[k] == c; }
    bool bad(const char *why) const { g_err = std::string(prefix) + why + " in SAM line '" + std::string(l, std::min<size_t>((size_t)(e - l), 80)) + "'"; return false; }
    bool split(const char *prefix_, const char *l_, const char *e_)
    {
        prefix = prefix_; l = l_; e = e_; nf = 0;
        f[nf++] = l;
        for (const char *p = l; p < e && nf < 12; ++p) if (*p == '\t') f[nf++] = p + 1;
        return nf < 11 ? bad("fewer than 11 fields") : true;
    }
    bool numbers()
    {
        if (!field_int(f[1], fe(1), &flag) || !field_int(f[3], fe(3), &pos1) || !field_int(f[4], fe(4), &mapq) || flag < 0 || flag > 0xFFFF || mapq < 0 || mapq > 255 ||
            pos1 < 0 || pos1 > 0x7FFFFFFF) return bad("a numeric field is no number of its range");
        return true;
    }
    bool parse(const char *prefix_, const char *l_, const char *e_) { return split(prefix_, l_, e_) && numbers(); }
};

// f(l, e) for every record line of sam[0 .. n): not empty (a skipped read, the paired-end driver's blank lines) and, with skip_headers, no
// '@' line (a read name cannot start with '@': the FASTQ parsers drop it).  The sum of what f returned, or its first negative value.
template <class F> int64_t for_record_lines(const char *sam, size_t n, bool skip_headers, F f)
{
    int64_t sum = 0;
    for (const char *l = sam, *end = sam + n; l < end; ) {
        const char *e = (const char *)memchr(l, '\n', (size_t)(end - l));
        if (!e) e = end;
        if (e > l && !(skip_headers && *l == '@')) {
            const int64_t r = f(l, e);
            if (r < 0) return r;
            sum += r;
        }
        l = e + 1;
    }
    return sum;
}

// one line -> one record appended to o; false with g_err set.  The read name is checked in front of the numbers.
bool bam_record_of_line(const RefIds &ids, const char *l, const char *e, Bytes &o)
{
    SamLine L;
    if (!L.split("BAM: ", l, e)) return false;
    const char *const *f = L.f; const int nf = L.nf;
    auto bad = [&](const char *why) { return L.bad(why); };
    auto fe = [&](int k) { return L.fe(k); };
    const size_t l_name = L.len(0);
    if (l_name == 0) return bad("empty read name");
    if (l_name > SALT_BAM_MAX_NAME) {
        g_err = "BAM: read name of " + std::to_string(l_name) + " bytes ('" + std::string(l, 40) + "...'): a BAM read name holds at most " +
                std::to_string(SALT_BAM_MAX_NAME) + " bytes";
        return false;
    }
    if (!L.numbers()) return false;
    const int64_t flag = L.flag, pos1 = L.pos1, mapq = L.mapq;
    int64_t pnext1, tlen;
    if (!field_int(f[7], fe(7), &pnext1) || !field_int(f[8], fe(8), &tlen) || pnext1 < 0 || pnext1 > 0x7FFFFFFF || tlen < INT32_MIN || tlen > INT32_MAX)
        return bad("a numeric field is no number of its range");
    int32_t rid = -1, nrid = -1;
    if (!(fe(2) - f[2] == 1 && *f[2] == '*') && (rid = ids.find(f[2], fe(2))) < -1) return bad("RNAME is no sequence of the index");
    if (fe(6) - f[6] == 1 && *f[6] == '=') nrid = rid;
    else if (!(fe(6) - f[6] == 1 && *f[6] == '*') && (nrid = ids.find(f[6], fe(6))) < -1) return bad("RNEXT is no sequence of the index");
    // CIGAR
    std::vector<uint32_t> cig;
    int64_t ref_len = 0;
    if (!(fe(5) - f[5] == 1 && *f[5] == '*')) {
        uint64_t n = 0; bool digits = false;
        for (const char *p = f[5]; p < fe(5); ++p) {
            if (*p >= '0' && *p <= '9') { n = 10 * n + (uint64_t)(*p - '0'); digits = true; if (n >= (1u << 28)) return bad("CIGAR length of 2^28 or more"); continue; }
            const char *ops = "MIDNSHP=X", *w = strchr(ops, *p);
            if (!w || !digits) return bad("malformed CIGAR");
            const uint32_t op = (uint32_t)(w - ops);
            cig.push_back((uint32_t)n << 4 | op);
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += (int64_t)n;
            n = 0; digits = false;
        }
        if (digits || cig.empty() || cig.size() > 0xFFFF) return bad("malformed CIGAR");
    }
    const int64_t pos = pos1 - 1;
    const uint32_t bin = pos < 0 ? 4680u : reg2bin(pos, pos + (ref_len > 0 ? ref_len : 1));
    const char *seq = f[9], *qual = f[10];
    size_t l_seq = (size_t)(fe(9) - seq);
    if (l_seq == 1 && *seq == '*') l_seq = 0;
    const size_t l_qual = (size_t)(fe(10) - qual);
    const bool no_qual = l_qual == 1 && *qual == '*' && l_seq != 1;
    if (!no_qual && l_qual != l_seq) return bad("SEQ and QUAL differ in length");
    const size_t at = o.b.size();
    o.u32(0);                                                      // block_size, set below
    o.u32((uint32_t)rid); o.u32((uint32_t)(int32_t)pos);
    o.u8((uint32_t)l_name + 1); o.u8((uint32_t)mapq); o.u16(bin);
    o.u16((uint32_t)cig.size()); o.u16((uint32_t)flag);
    o.u32((uint32_t)l_seq);
    o.u32((uint32_t)nrid); o.u32((uint32_t)(int32_t)(pnext1 - 1)); o.u32((uint32_t)(int32_t)tlen);
    o.text(f[0], fe(0)); o.u8(0);
    for (uint32_t c : cig) o.u32(c);
    auto code = [](char c) -> uint32_t {                           // "=ACMGRSVTWYHKDBN"
        switch (c) { case '=': return 0; case 'A': case 'a': return 1; case 'C': case 'c': return 2; case 'M': case 'm': return 3; case 'G': case 'g': return 4;
                     case 'R': case 'r': return 5; case 'S': case 's': return 6; case 'V': case 'v': return 7; case 'T': case 't': return 8; case 'W': case 'w': return 9;
                     case 'Y': case 'y': return 10; case 'H': case 'h': return 11; case 'K': case 'k': return 12; case 'D': case 'd': return 13; case 'B': case 'b': return 14;
                     default: return 15; }
    };
    for (size_t i = 0; i < l_seq; i += 2) o.u8(code(seq[i]) << 4 | (i + 1 < l_seq ? code(seq[i + 1]) : 0u));
    for (size_t i = 0; i < l_seq; ++i) {
        if (no_qual) { o.u8(0xFF); continue; }
        if ((unsigned char)qual[i] < 33 || (unsigned char)qual[i] > 126) return bad("a quality character outside '!' .. '~'");
        o.u8((uint32_t)((unsigned char)qual[i] - 33));
    }
    // tags: TAG:TYPE:VALUE
    for (const char *t = nf > 11 ? f[11] : e; t < e; ) {
        const char *te = (const char *)memchr(t, '\t', (size_t)(e - t));
        if (!te) te = e;
        if (te - t < 5 || t[2] != ':' || t[4] != ':') return bad("malformed tag");
        const char *v = t + 5;
        o.u8((unsigned char)t[0]); o.u8((unsigned char)t[1]);
        if (t[0] == 'X' && t[1] == 'V' && t[3] == 'i') {           // the offsets of the listed alleles: one tag, one type, however many there are
            std::vector<uint32_t> items;
            for (const char *p = v; p <= te; ) {
                const char *c = (const char *)memchr(p, ',', (size_t)(te - p));
                if (!c) c = te;
                int64_t x;
                if (!field_int(p, c, &x) || x < 0 || x > 0xFFFFFFFFll) return bad("malformed XV list");
                items.push_back((uint32_t)x);
                p = c + 1;
            }
            o.u8('B'); o.u8('I'); o.u32((uint32_t)items.size());
            for (uint32_t x : items) o.u32(x);
        } else if (t[3] == 'Z') { o.u8('Z'); o.text(v, te); o.u8(0); }
        else if (t[3] == 'i') {
            int64_t x;
            if (!field_int(v, te, &x) || x < INT32_MIN || x > 0xFFFFFFFFll) return bad("malformed integer tag");
            bam_int_tag(o, x);
        } else return bad("a tag type this program does not write");
        t = te + 1;
    }
    o.set32(at, (uint32_t)(o.b.size() - at - 4));
    return true;
}

} // namespace

extern "C" int64_t salt_bam_header(const salt_index_t *ix, const char *header_text, size_t n_text, uint8_t *out, size_t cap)
{
    if (!ix || (!header_text && n_text) || n_text > 0x7FFFFFFFu) { g_err = "BAM: bad header arguments"; return SALT_BAM_E_INVAL; }
    Bytes o;
    o.u8('B'); o.u8('A'); o.u8('M'); o.u8(1);
    o.u32((uint32_t)n_text); o.text(header_text, header_text + n_text);
    o.u32((uint32_t)ix->anns.size());
    for (const Ann &a : ix->anns) { o.u32((uint32_t)a.name.size() + 1); o.text(a.name.data(), a.name.data() + a.name.size()); o.u8(0); o.u32((uint32_t)a.len); }
    if (o.b.size() > cap || !out) return SALT_BAM_E_CAP;
    memcpy(out, o.b.data(), o.b.size());
    return (int64_t)o.b.size();
}

extern "C" int64_t salt_bam_from_sam(const salt_index_t *ix, const char *sam, size_t n, uint8_t *out, size_t cap, uint64_t *n_records)
{
    if (n_records) *n_records = 0;
    if (!ix || (!sam && n) || (!out && cap)) { g_err = "BAM: null argument"; return SALT_BAM_E_INVAL; }
    const RefIds ids(ix);
    Bytes rec;
    size_t w = 0;
    const int64_t n_rec = for_record_lines(sam, n, false, [&](const char *l, const char *e) -> int64_t {
        rec.b.clear();
        if (!bam_record_of_line(ids, l, e, rec)) return SALT_BAM_E_INVAL;
        if (w + rec.b.size() > cap) return SALT_BAM_E_CAP;
        memcpy(out + w, rec.b.data(), rec.b.size());
        w += rec.b.size();
        return 1;
    });
    if (n_rec < 0) return n_rec;
    if (n_records) *n_records = (uint64_t)n_rec;
    return (int64_t)w;
}

// ---------------------------------------------------------------------------------------------
// Allele counts at the SNP sites: the host twin of the device's site table and k_snp_count (include/salt_gpu.h has the definition), written
// from that definition over this program's own SAM record lines and without any code of the kernel's.
// ---------------------------------------------------------------------------------------------
namespace {

const std::vector<uint32_t> &snp_positions(const salt_index *ix)
{
    std::call_once(ix->snp_once, [ix]() {
        for (uint32_t g = 0; g < ix->view.ref_len; ++g) {
            const uint32_t m = mask_at(ix, g);
            if (m & (m - 1u)) ix->snp_pos.push_back(g);                // two or more bases listed (an N of the genome has mask 0)
        }
    });
    return ix->snp_pos;
}

// ---- what the three twins share (with each other, and with nothing under csrc/) ----
// The M runs of a counted record line: genome positions [g, g + len), bases [s, s + len) of SEQ; gapped: the CIGAR has an I, S or D.
struct MRuns { uint64_t g[64], len[64]; size_t s[64]; int n = 0; bool gapped = false; };

// The line's head: 1 it counts and *g is its global position, 0 it does not (unmapped, also a mate printed at its mate's place: flag & 4;
// else below min_mapq), -1 with g_err set.
int twin_head(const salt_index *ix, const RefIds &ids, SamLine &L, const char *prefix, const char *l, const char *e, uint32_t min_mapq, uint64_t *g)
{
    if (!L.parse(prefix, l, e)) return -1;
    if ((L.flag & 4) || (uint64_t)L.mapq < min_mapq) return 0;
    const int32_t rid = ids.find(L.f[2], L.fe(2));
    if (rid < 0) return L.bad("RNAME is no sequence of the index"), -1;
    if (L.pos1 < 1) return L.bad("a mapped record without a position"), -1;
    *g = (uint64_t)ix->anns[(size_t)rid].offset + (uint64_t)L.pos1 - 1;            // the walk may run past the contig's end
    return 1;
}
// The line's CIGAR, checked whole against SEQ before the caller adds anything: a refused line leaves the caller's table as it was.
bool twin_cigar(const SamLine &L, uint64_t g, MRuns &m)
{
    const size_t l_seq = L.len(9);
    size_t s = 0; uint64_t n = 0; bool digits = false, any = false;
    for (const char *p = L.f[5]; p < L.fe(5); ++p) {
        if (*p >= '0' && *p <= '9') { n = 10 * n + (uint64_t)(*p - '0'); digits = true; if (n >= (1u << 28)) return L.bad("CIGAR length of 2^28 or more"); continue; }
        if (!digits) return L.bad("malformed CIGAR");
        switch (*p) {
        case 'M':
            if (s + n > l_seq) return L.bad("the CIGAR is longer than SEQ");
            if (m.n == 64) return L.bad("more M runs than a record of this program has");
            m.g[m.n] = g; m.s[m.n] = s; m.len[m.n] = n; ++m.n;
            g += n; s += n; break;
        case 'I': case 'S':
            if (s + n > l_seq) return L.bad("the CIGAR is longer than SEQ");
            s += n; m.gapped = true; break;
        case 'D': g += n; m.gapped = true; break;
        default: return L.bad("a CIGAR operation this program does not write");
        }
        n = 0; digits = false; any = true;
    }
    return digits || !any ? L.bad("malformed CIGAR") : true;
}
inline int base_code(char c) { switch (c) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return -1; } }

// one record line [l, e): its bases at the sites into counts; 1 it contributed, 0 it did not (unmapped, below min_mapq), -1 with g_err set
int snp_count_line(const salt_index *ix, const RefIds &ids, const std::vector<uint32_t> &sites, const char *l, const char *e, uint32_t min_mapq, uint32_t *counts)
{
    SamLine L; MRuns m; uint64_t g0;
    const int h = twin_head(ix, ids, L, "snp counts: ", l, e, min_mapq, &g0);
    if (h != 1) return h;
    if (!twin_cigar(L, g0, m)) return -1;
    for (int r = 0; r < m.n; ++r)
        for (uint64_t k = 0; k < m.len[r]; ++k) {
            const uint64_t g = m.g[r] + k;
            const auto it = std::lower_bound(sites.begin(), sites.end(), g);
            if (g > 0xFFFFFFFFull || it == sites.end() || *it != g) continue;
            const int b = base_code(L.f[9][m.s[r] + k]);
            if (b >= 0) ++counts[(size_t)(it - sites.begin()) * 4 + (size_t)b];
        }
    return 1;
}

} // namespace

extern "C" int64_t salt_snp_sites(const salt_index_t *ix, uint32_t *pos, uint64_t cap)
{
    if (!ix) { g_err = "snp counts: null argument"; return -1; }
    const std::vector<uint32_t> &sites = snp_positions(ix);
    if (pos) memcpy(pos, sites.data(), (size_t)std::min<uint64_t>(cap, sites.size()) * 4);
    return (int64_t)sites.size();
}

extern "C" int64_t salt_snp_count_sam(const salt_index_t *ix, const char *sam, size_t n, uint32_t min_mapq, uint32_t *counts, uint64_t n_sites)
{
    if (!ix || (!sam && n) || !counts) { g_err = "snp counts: null argument"; return -1; }
    const std::vector<uint32_t> &sites = snp_positions(ix);
    if (n_sites != sites.size()) { g_err = "snp counts: counts for " + std::to_string(n_sites) + " sites, the index has " + std::to_string(sites.size()); return -1; }
    const RefIds ids(ix);
    return for_record_lines(sam, n, true, [&](const char *l, const char *e) { return snp_count_line(ix, ids, sites, l, e, min_mapq, counts); });
}

// ---------------------------------------------------------------------------------------------
// Coverage: the host twin of the device's difference array and text kernels (k_depth_mark, salt_depth.hip; include/salt_gpu.h has the
// definition), written from that definition over this program's own SAM record lines and without any code of the kernels'.
// ---------------------------------------------------------------------------------------------
namespace {

// one record line [l, e): its M runs into diff; 1 it contributed, 0 it did not (unmapped, below min_mapq), -1 with g_err set
int depth_add_line(const salt_index *ix, const RefIds &ids, const char *l, const char *e, uint32_t min_mapq, uint32_t *diff)
{
    SamLine L; MRuns m; uint64_t g0;
    const int h = twin_head(ix, ids, L, "depth: ", l, e, min_mapq, &g0);
    if (h != 1) return h;
    if (!twin_cigar(L, g0, m)) return -1;
    for (int k = 0; k < m.n; ++k) {
        const uint64_t a = m.g[k], b = std::min<uint64_t>(a + m.len[k], ix->view.ref_len);      // cut at the genome's end: not wrapped, not refused
        if (a < b) { diff[a] += 1u; diff[b] -= 1u; }
    }
    return 1;
}

struct DepthOut {                                                      // counts every byte, keeps those that fit
    char *p; uint64_t cap, n = 0;
    void put(char c) { if (n < cap) p[n] = c; ++n; }
    void puts(const std::string &s) { for (char c : s) put(c); }
    void putu(uint64_t v) { char b[24]; int k = 0; do { b[k++] = (char)('0' + v % 10); v /= 10; } while (v); while (k) put(b[--k]); }
};

} // namespace

extern "C" int64_t salt_depth_add_sam(const salt_index_t *ix, const char *sam, size_t n, uint32_t min_mapq, uint32_t *diff, uint64_t n_words)
{
    if (!ix || (!sam && n) || !diff) { g_err = "depth: null argument"; return -1; }
    if (n_words != (uint64_t)ix->view.ref_len + 1) { g_err = "depth: an array of " + std::to_string(n_words) + " words, the index needs " + std::to_string((uint64_t)ix->view.ref_len + 1) + " (ref_len + 1)"; return -1; }
    const RefIds ids(ix);
    return for_record_lines(sam, n, true, [&](const char *l, const char *e) { return depth_add_line(ix, ids, l, e, min_mapq, diff); });
}

extern "C" int64_t salt_depth_text(const salt_index_t *ix, const uint32_t *diff, uint64_t n_words, uint32_t window, char *out, uint64_t cap)
{
    if (!ix || !diff || (!out && cap)) { g_err = "depth: null argument"; return -1; }
    const uint64_t ref_len = ix->view.ref_len;
    if (n_words != ref_len + 1) { g_err = "depth: an array of " + std::to_string(n_words) + " words, the index needs " + std::to_string(ref_len + 1) + " (ref_len + 1)"; return -1; }
    DepthOut o{ out, cap };
    uint32_t depth = 0;                                                // depth[g - 1] in front of position g, mod 2^32
    for (size_t c = 0; c < ix->anns.size(); ++c) {
        const uint64_t c0 = (uint64_t)ix->anns[c].offset, c1 = c + 1 < ix->anns.size() ? std::min<uint64_t>((uint64_t)ix->anns[c + 1].offset, ref_len) : ref_len;
        const std::string &name = ix->anns[c].name;
        if (c0 >= c1) continue;
        if (window == 0) {
            uint64_t start = c0; uint32_t d_run = depth + diff[c0];
            for (uint64_t g = c0; g < c1; ++g) {
                depth += diff[g];
                if (depth != d_run) {
                    o.puts(name); o.put('\t'); o.putu(start - c0); o.put('\t'); o.putu(g - c0); o.put('\t'); o.putu(d_run); o.put('\n');
                    start = g; d_run = depth;
                }
            }
            o.puts(name); o.put('\t'); o.putu(start - c0); o.put('\t'); o.putu(c1 - c0); o.put('\t'); o.putu(d_run); o.put('\n');
        } else {
            for (uint64_t w0 = c0; w0 < c1; w0 += window) {
                const uint64_t w1 = std::min<uint64_t>(w0 + window, c1), len = w1 - w0;
                uint64_t sum = 0;
                for (uint64_t g = w0; g < w1; ++g) { depth += diff[g]; sum += depth; }
                // h = (100 sum + len / 2) / len without leaving 64 bits: sum = q len + r gives 100 q + (100 r + len / 2) / len
                const uint64_t h = 100u * (sum / len) + (100u * (sum % len) + len / 2) / len;
                o.puts(name); o.put('\t'); o.putu(w0 - c0); o.put('\t'); o.putu(w1 - c0); o.put('\t'); o.putu((uint64_t)(h / 100u)); o.put('.');
                o.put((char)('0' + (int)(h % 100u) / 10)); o.put((char)('0' + (int)(h % 100u) % 10)); o.put('\n');
            }
        }
    }
    return (int64_t)o.n;
}

// ---------------------------------------------------------------------------------------------
// The error profile: the host twin of k_errprof (salt_errprof.hip; include/salt_gpu.h has the definition), written from that definition
// over this program's own SAM record lines and without any code of the kernel's, and the printer of the file.
// ---------------------------------------------------------------------------------------------
namespace {

const uint64_t EP_CYCLES = 512, EP_Q = 95, EP_CELLS = 2 * EP_CYCLES * EP_Q * 16;

// one record line [l, e): its base events into cells, its fate into rec; 1 it counted, 0 it did not (unmapped, below min_mapq), -1 with g_err set
int errprof_add_line(const salt_index *ix, const RefIds &ids, const char *l, const char *e, uint32_t min_mapq, uint64_t *cells, uint64_t *rec)
{
    SamLine L; MRuns m; uint64_t g0;
    const int h = twin_head(ix, ids, L, "error profile: ", l, e, min_mapq, &g0);
    if (h < 0) return h;
    uint64_t *r = rec + ((L.flag & 0x80) ? 8 : 0);
    const uint64_t mate = (L.flag & 0x80) ? 1 : 0;
    if (h == 0) { ++r[0]; ++r[(L.flag & 4) ? 2 : 3]; return 0; }
    const bool rev = (L.flag & 0x10) != 0;
    const char *seq = L.f[9], *qual = L.f[10]; const size_t l_seq = L.len(9), l_qual = L.len(10);
    if (l_seq == 0 || l_seq > EP_CYCLES) return L.bad("SEQ is empty or longer than 512 bases"), -1;
    const bool no_qual = l_qual == 1 && qual[0] == '*' && l_seq != 1;
    if (!no_qual && l_qual != l_seq) return L.bad("QUAL is neither * nor as long as SEQ"), -1;
    if (!twin_cigar(L, g0, m)) return -1;
    for (int k = 0; k < m.n; ++k)
        for (uint64_t j = 0; j < m.len[k]; ++j) {
            const uint64_t g = m.g[k] + j; const size_t s = m.s[k] + j;
            if (g >= ix->view.ref_len) continue;
            const uint32_t mk = mask_at(ix, (uint32_t)g);
            if (mk == 0 || (mk & (mk - 1u)) != 0) continue;                    // N of the genome; a site
            const int b = base_code(seq[s]);
            if (b < 0) continue;                                               // a read's N
            int c = 0; while (!((mk >> c) & 1u)) ++c;
            const uint32_t q = no_qual ? 94u : ((uint8_t)qual[s] >= 33 && (uint8_t)qual[s] <= 126 ? (uint32_t)(uint8_t)qual[s] - 33u : 94u);
            const uint64_t cycle = rev ? l_seq - 1 - s : s;
            ++cells[((mate * EP_CYCLES + cycle) * EP_Q + q) * 16 + (uint64_t)(rev ? 3 - c : c) * 4 + (uint64_t)(rev ? 3 - b : b)];
        }
    ++r[0]; ++r[4];
    if (rev) ++r[5];
    if (m.gapped) ++r[6];
    return 1;
}

} // namespace

extern "C" int64_t salt_errprof_add_sam(const salt_index_t *ix, const char *sam, size_t n, uint32_t min_mapq, uint64_t *cells, uint64_t n_cells, uint64_t rec[16])
{
    if (!ix || (!sam && n) || !cells || !rec) { g_err = "error profile: null argument"; return -1; }
    if (n_cells != EP_CELLS) { g_err = "error profile: a table of " + std::to_string(n_cells) + " cells, the profile has " + std::to_string(EP_CELLS) + " (2 x 512 x 95 x 4 x 4)"; return -1; }
    const RefIds ids(ix);
    return for_record_lines(sam, n, true, [&](const char *l, const char *e) { return errprof_add_line(ix, ids, l, e, min_mapq, cells, rec); });
}

extern "C" int64_t salt_errprof_text(const uint64_t *cells, const uint64_t rec[16], uint32_t min_mapq, int full, char *out, uint64_t cap)
{
    if (!cells || !rec || (!out && cap)) { g_err = "error profile: null argument"; return -1; }
    DepthOut o{ out, cap };
    static const char NT[] = "ACGT";
    auto cell = [&](uint64_t mate, uint64_t cyc, uint64_t q, uint64_t rr) { return cells[((mate * EP_CYCLES + cyc) * EP_Q + q) * 16 + rr]; };
    auto row = [&](char tag, uint64_t mate) { o.put(tag); o.put('\t'); o.putu(mate); };
    auto num = [&](uint64_t v) { o.put('\t'); o.putu(v); };
    const bool show[2] = { rec[0] != 0, rec[8] != 0 };
    o.puts("#salt-error-profile\tv1\tmin_mapq="); o.putu(min_mapq); o.put('\n');
    o.puts("#R\tmate\tseen\tskipped\tunmapped\tlow_mapq\tcounted\treverse\tgapped\n");
    for (uint64_t m = 0; m < 2; ++m) if (show[m]) { row('R', m); for (int k = 0; k < 7; ++k) num(rec[m * 8 + (uint64_t)k]); o.put('\n'); }
    o.puts("#Q\tmate\tq\tbases\tmismatches\tempirical\n");
    for (uint64_t m = 0; m < 2; ++m) if (show[m])
        for (uint64_t q = 0; q < EP_Q; ++q) {
            uint64_t bases = 0, mm = 0;
            for (uint64_t c = 0; c < EP_CYCLES; ++c) for (uint64_t rr = 0; rr < 16; ++rr) { const uint64_t v = cell(m, c, q, rr); bases += v; if ((rr >> 2) != (rr & 3)) mm += v; }
            if (!bases) continue;
            row('Q', m); o.put('\t');
            if (q == EP_Q - 1) o.puts("none"); else o.putu(q);
            num(bases); num(mm);
            char b[64]; snprintf(b, sizeof b, "\t%.2f\n", -10.0 * log10(((double)mm + 1.0) / ((double)bases + 2.0)));
            o.puts(b);
        }
    o.puts("#C\tmate\tcycle\tbases\tmismatches\n");
    for (uint64_t m = 0; m < 2; ++m) if (show[m])
        for (uint64_t c = 0; c < EP_CYCLES; ++c) {
            uint64_t bases = 0, mm = 0;
            for (uint64_t q = 0; q < EP_Q; ++q) for (uint64_t rr = 0; rr < 16; ++rr) { const uint64_t v = cell(m, c, q, rr); bases += v; if ((rr >> 2) != (rr & 3)) mm += v; }
            if (!bases) continue;
            row('C', m); num(c + 1); num(bases); num(mm); o.put('\n');
        }
    o.puts("#S\tmate\tref\tread\tcount\n");
    for (uint64_t m = 0; m < 2; ++m) if (show[m])
        for (uint64_t rr = 0; rr < 16; ++rr) {
            uint64_t v = 0;
            for (uint64_t c = 0; c < EP_CYCLES; ++c) for (uint64_t q = 0; q < EP_Q; ++q) v += cell(m, c, q, rr);
            row('S', m); o.put('\t'); o.put(NT[rr >> 2]); o.put('\t'); o.put(NT[rr & 3]); num(v); o.put('\n');
        }
    if (full) {
        o.puts("#E\tmate\tcycle\tq\tref\tread\tcount\n");
        for (uint64_t m = 0; m < 2; ++m) if (show[m])
            for (uint64_t c = 0; c < EP_CYCLES; ++c) for (uint64_t q = 0; q < EP_Q; ++q) for (uint64_t rr = 0; rr < 16; ++rr) {
                const uint64_t v = cell(m, c, q, rr);
                if (!v) continue;
                row('E', m); num(c + 1); o.put('\t');
                if (q == EP_Q - 1) o.puts("none"); else o.putu(q);
                o.put('\t'); o.put(NT[rr >> 2]); o.put('\t'); o.put(NT[rr & 3]); num(v); o.put('\n');
            }
    }
    return (int64_t)o.n;
}

// ---------------------------------------------------------------------------------------------
// Genotypes at the SNP sites: the host twin of k_gt_add and of the device's call and text kernels (salt_gt.hip; include/salt_gpu.h has the
// definition), written from that definition over this program's own SAM record lines.  It shares the penalty table's header with the
// kernels and nothing else.
// ---------------------------------------------------------------------------------------------
#include "../../include/salt_gt_table.h"

namespace {

// one record line [l, e): its events into sites; 1 it contributed, 0 it did not (unmapped, below min_mapq), -1 with g_err set.  The line is
// checked whole (head, QUAL's length, CIGAR) before anything is added.
int gt_add_line(const salt_index *ix, const RefIds &ids, const std::vector<uint32_t> &pos, const char *l, const char *e, uint32_t min_mapq, salt_gt_site_t *sites)
{
    SamLine L; MRuns m; uint64_t g0;
    const int h = twin_head(ix, ids, L, "genotype: ", l, e, min_mapq, &g0);
    if (h != 1) return h;
    const char *seq = L.f[9], *qual = L.f[10]; const size_t l_seq = L.len(9), l_qual = L.len(10);
    const bool no_qual = l_qual == 1 && qual[0] == '*' && l_seq != 1;
    if (!no_qual && l_qual != l_seq) return L.bad("QUAL is neither * nor as long as SEQ"), -1;
    if (!twin_cigar(L, g0, m)) return -1;
    for (int r = 0; r < m.n; ++r)
        for (uint64_t k = 0; k < m.len[r]; ++k) {
            const uint64_t g = m.g[r] + k; const size_t s = m.s[r] + k;
            const auto it = std::lower_bound(pos.begin(), pos.end(), g);
            if (g > 0xFFFFFFFFull || it == pos.end() || *it != g) continue;
            const int b = base_code(seq[s]);
            if (b < 0) continue;
            const uint8_t qb = no_qual ? 0 : (uint8_t)qual[s];
            const uint32_t q = qb >= 33 && qb <= 126 ? (uint32_t)qb - 33u : (uint32_t)SALT_GT_Q_NONE;
            salt_gt_base_t &w = sites[(size_t)(it - pos.begin())].b[b];
            w.n += 1; w.sm += SALT_GT_TABLE[q][0]; w.sx += SALT_GT_TABLE[q][1]; w.sh += SALT_GT_TABLE[q][2];
        }
    return 1;
}

} // namespace

extern "C" int64_t salt_gt_add_sam(const salt_index_t *ix, const char *sam, size_t n, uint32_t min_mapq, salt_gt_site_t *sites, uint64_t n_sites)
{
    if (!ix || (!sam && n) || !sites) { g_err = "genotype: null argument"; return -1; }
    const std::vector<uint32_t> &pos = snp_positions(ix);
    if (n_sites != pos.size()) { g_err = "genotype: sums for " + std::to_string(n_sites) + " sites, the index has " + std::to_string(pos.size()); return -1; }
    const RefIds ids(ix);
    return for_record_lines(sam, n, true, [&](const char *l, const char *e) { return gt_add_line(ix, ids, pos, l, e, min_mapq, sites); });
}

extern "C" int64_t salt_gt_text(const salt_index_t *ix, const salt_gt_site_t *sites, uint64_t first, uint64_t n, char *out, uint64_t cap)
{
    if (!ix || (!sites && n) || (!out && cap)) { g_err = "genotype: null argument"; return -1; }
    const std::vector<uint32_t> &pos = snp_positions(ix);
    if (first > pos.size() || n > pos.size() - first) {
        g_err = "genotype: sites [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") leave the index's [0, " + std::to_string(pos.size()) + ")";
        return -1;
    }
    DepthOut o{ out, cap };
    static const char NT[] = "ACGT";
    for (uint64_t i = 0; i < n; ++i) {
        const salt_gt_site_t &S = sites[i];                            // (sites[0] is site `first`)
        const uint32_t g = pos[(size_t)(first + i)];
        const uint32_t mask = mask_at(ix, g), r = (int64_t)g < ix->l_pac ? pac_at(ix, g) : 0u;
        int al[4], n_al = 0;
        al[n_al++] = (int)r;
        for (int b = 0; b < 4; ++b) if (((mask >> b) & 1u) && (uint32_t)b != r) al[n_al++] = b;
        uint64_t all_x = 0, dp = 0;
        for (int b = 0; b < 4; ++b) { all_x += S.b[b].sx; dp += S.b[b].n; }
        uint64_t raw[10]; int n_gt = 0, ga[10], gb[10];
        for (int b = 0; b < n_al; ++b)
            for (int a = 0; a <= b; ++a, ++n_gt) {                     // VCF order: b (b + 1) / 2 + a
                const salt_gt_base_t &A = S.b[al[a]], &B = S.b[al[b]];
                raw[n_gt] = a == b ? A.sm + (all_x - A.sx) : A.sh + B.sh + (all_x - A.sx - B.sx);
                ga[n_gt] = a; gb[n_gt] = b;
            }
        int best = 0;
        for (int k = 1; k < n_gt; ++k) if (raw[k] < raw[best]) best = k;      // the first of the smallest
        size_t c = 0;                                                  // the last contig that begins at or in front of g
        for (size_t k = 1; k < ix->anns.size(); ++k) if ((uint64_t)ix->anns[k].offset <= g) c = k;
        o.puts(ix->anns[c].name); o.put('\t'); o.putu((uint64_t)g - (uint64_t)ix->anns[c].offset + 1); o.puts("\t.\t");
        o.put(NT[r]); o.put('\t');
        for (int k = 1; k < n_al; ++k) { if (k > 1) o.put(','); o.put(NT[al[k]]); }
        o.put('\t');
        if (dp == 0) {
            o.puts(".\t.\tDP=0\tGT:AD:DP:GQ:PL\t./.:");
            for (int k = 0; k < n_al; ++k) { if (k) o.put(','); o.put('0'); }
            o.puts(":0:.:.\n");
            continue;
        }
        auto pl = [&](int k) { return (raw[k] - raw[best] + 2048u) >> 12; };
        uint64_t gq = ~0ull;
        for (int k = 0; k < n_gt; ++k) if (k != best) gq = std::min<uint64_t>(gq, pl(k));
        gq = std::min<uint64_t>(gq, 99);
        o.putu(pl(0)); o.puts("\t.\tDP="); o.putu(dp); o.puts("\tGT:AD:DP:GQ:PL\t");
        o.putu((uint64_t)ga[best]); o.put('/'); o.putu((uint64_t)gb[best]); o.put(':');
        for (int k = 0; k < n_al; ++k) { if (k) o.put(','); o.putu(S.b[al[k]].n); }
        o.put(':'); o.putu(dp); o.put(':'); o.putu(gq); o.put(':');
        for (int k = 0; k < n_gt; ++k) { if (k) o.put(','); o.putu(pl(k)); }
        o.put('\n');
    }
    return (int64_t)o.n;
}

extern "C" int64_t salt_gt_header(const salt_index_t *ix, const char *sample, char *out, uint64_t cap)
{
    if (!ix || (!out && cap)) { g_err = "genotype: null argument"; return -1; }
    const std::string name = sample && *sample ? sample : "sample";
    for (char ch : name) if (ch == '\t' || ch == '\n' || ch == '\r') { g_err = "genotype: the sample name holds a tab or a line end"; return -1; }
    DepthOut o{ out, cap };
    o.puts("##fileformat=VCFv4.2\n##source=salt --genotype\n");
    for (const Ann &a : ix->anns) { o.puts("##contig=<ID="); o.puts(a.name); o.puts(",length="); o.putu((uint64_t)a.len); o.puts(">\n"); }
    o.puts("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Bases of counted reads at the site (A, C, G, T)\">\n"
           "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
           "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Bases that show each allele\">\n"
           "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Bases of counted reads at the site (A, C, G, T)\">\n"
           "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: the smallest PL of another genotype, at most 99\">\n"
           "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods, flat priors, uncapped\">\n"
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t");
    o.puts(name); o.put('\n');
    return (int64_t)o.n;
}

extern "C" const uint32_t *salt_gt_table(void) { return &SALT_GT_TABLE[0][0]; }

// ---------------------------------------------------------------------------------------------
// SNP candidates off the index's sites: the host twin of k_disc_add and of the device's flag and line kernels (salt_discover.hip;
// include/salt_gpu.h has the definition), written from that definition over this program's own SAM record lines.  It shares nothing with
// anything under csrc/.
// ---------------------------------------------------------------------------------------------
namespace {

// one record line [l, e): its M runs into diff, its events into alt; 1 it contributed, 0 it did not (unmapped, below min_mapq), -1 with
// g_err set.  The line is checked whole (head, QUAL's length, CIGAR) before anything is added.
int disc_add_line(const salt_index *ix, const RefIds &ids, const char *l, const char *e, uint32_t min_mapq, uint32_t min_baseq, uint64_t *alt, uint32_t *diff)
{
    SamLine L; MRuns m; uint64_t g0;
    const int h = twin_head(ix, ids, L, "discover: ", l, e, min_mapq, &g0);
    if (h != 1) return h;
    const char *seq = L.f[9], *qual = L.f[10]; const size_t l_seq = L.len(9), l_qual = L.len(10);
    const bool no_qual = l_qual == 1 && qual[0] == '*' && l_seq != 1;
    if (!no_qual && l_qual != l_seq) return L.bad("QUAL is neither * nor as long as SEQ"), -1;
    if (!twin_cigar(L, g0, m)) return -1;
    const uint64_t ref_len = ix->view.ref_len;
    for (int r = 0; r < m.n; ++r) {
        const uint64_t a = m.g[r], b = std::min<uint64_t>(a + m.len[r], ref_len);      // cut at the genome's end: not wrapped, not refused
        if (a >= b) continue;
        diff[a] += 1u; diff[b] -= 1u;
        for (uint64_t g = a; g < b; ++g) {
            const size_t s = m.s[r] + (size_t)(g - a);
            const int base = base_code(seq[s]);
            if (base < 0) continue;                                            // a read's N
            const uint32_t mk = mask_at(ix, (uint32_t)g);
            if (mk == 0 || ((mk >> base) & 1u)) continue;                      // N of the genome; a base the index has there
            const uint8_t qb = no_qual ? 0 : (uint8_t)qual[s];
            if (qb >= 33 && qb <= 126 && (uint32_t)qb - 33u < min_baseq) continue;      // a usable quality below the floor
            int k = 0;
            for (int c = 0; c < base; ++c) if (!((mk >> c) & 1u)) ++k;         // the rank of the base among those outside the mask
            alt[g] += 1ull << (SALT_DISC_FIELD_BITS * k);
        }
    }
    return 1;
}

bool disc_sizes(const salt_index *ix, uint64_t n_pos)
{
    if (n_pos == ix->view.ref_len) return true;
    g_err = "discover: arrays for " + std::to_string(n_pos) + " positions, the index has " + std::to_string((uint64_t)ix->view.ref_len) + " (alt: ref_len words, diff: ref_len + 1)";
    return false;
}

} // namespace

extern "C" int64_t salt_disc_add_sam(const salt_index_t *ix, const char *sam, size_t n, uint32_t min_mapq, uint32_t min_baseq, uint64_t *alt, uint32_t *diff, uint64_t n_pos)
{
    if (!ix || (!sam && n) || !alt || !diff) { g_err = "discover: null argument"; return -1; }
    if (!disc_sizes(ix, n_pos)) return -1;
    const RefIds ids(ix);
    return for_record_lines(sam, n, true, [&](const char *l, const char *e) { return disc_add_line(ix, ids, l, e, min_mapq, min_baseq, alt, diff); });
}

extern "C" int64_t salt_disc_text(const salt_index_t *ix, const uint64_t *alt, const uint32_t *diff, uint64_t n_pos, uint32_t min_alt, uint32_t min_pct, int all_sites,
                                  char *out, uint64_t cap, uint8_t *seen)
{
    if (!ix || !alt || !diff || (!out && cap)) { g_err = "discover: null argument"; return -1; }
    if (!disc_sizes(ix, n_pos)) return -1;
    if (min_alt < 1 || min_alt > SALT_DISC_FIELD_MAX || min_pct > 100) { g_err = "discover: min_alt is 1 .. 2097151 and min_pct 0 .. 100"; return -1; }
    DepthOut o{ out, cap };
    static const char NT[] = "ACGT";
    if (seen) memset(seen, 0, ix->anns.size());
    uint32_t depth = 0;                                                // the prefix sum of diff, mod 2^32
    size_t c = 0;                                                      // the last contig that begins at or in front of g
    for (uint64_t g = 0; g < n_pos; ++g) {
        depth += diff[g];
        const uint64_t w = alt[g];
        if (w == 0 && !all_sites) continue;
        const uint32_t mk = mask_at(ix, (uint32_t)g);
        if (mk == 0) continue;
        uint32_t called = 0; uint64_t cnt[4] = { 0, 0, 0, 0 };
        for (int b = 0, k = 0; b < 4; ++b) {
            if ((mk >> b) & 1u) continue;
            cnt[b] = (w >> (SALT_DISC_FIELD_BITS * k++)) & SALT_DISC_FIELD_MAX;
            if (cnt[b] >= min_alt && 100 * cnt[b] >= (uint64_t)min_pct * depth) called |= 1u << b;
        }
        if (!called && !(all_sites && (mk & (mk - 1u)))) continue;
        while (c + 1 < ix->anns.size() && (uint64_t)ix->anns[c + 1].offset <= g) ++c;
        if (seen) seen[c] = 1;
        o.puts(ix->anns[c].name); o.put('\t'); o.putu(g - (uint64_t)ix->anns[c].offset + 1); o.put('\t');
        bool first = true;
        for (int b = 0; b < 4; ++b) if (((mk | called) >> b) & 1u) { if (!first) o.put('/'); o.put(NT[b]); first = false; }
        o.put('\t'); o.put(NT[(int64_t)g < ix->l_pac ? pac_at(ix, (uint32_t)g) : 0u]); o.put('\t'); o.putu(depth); o.put('\t');
        for (int b = 0; b < 4; ++b) { if (b) o.put(','); if ((mk >> b) & 1u) o.put('.'); else o.putu(cnt[b]); }
        o.put('\n');
    }
    return (int64_t)o.n;
}

// ---------------------------------------------------------------------------------------------
// The run's summary: the host twin of k_stats_add (salt_stats.hip; include/salt_gpu.h has the definition), written from that definition
// over this program's own SAM record lines and without any code of the kernel's, and the printer of the file.
// ---------------------------------------------------------------------------------------------
namespace {

const uint64_t ST_SN = 0, ST_MQ = 32, ST_RL = 544, ST_GC = 1570, ST_XA = 1774, ST_IS = 1790, ST_OR = 5887, ST_ID = 5891, ST_CELLS = 6021, ST_IS_MAX = 4096;

bool stats_sizes(const salt_index *ix, uint64_t n_cells, uint64_t n_ct)
{
    if (n_cells == ST_CELLS && n_ct == 8 * (uint64_t)ix->anns.size()) return true;
    g_err = "stats: tables of " + std::to_string(n_cells) + " and " + std::to_string(n_ct) + " cells, the summary has " + std::to_string(ST_CELLS) + " fixed cells and 8 for each of the index's " +
            std::to_string(ix->anns.size()) + " sequences";
    return false;
}

// one record line [l, e) into the tables; 1 it counted, 0 it did not (unmapped, below min_mapq), -1 with g_err set.  The line is checked
// whole (head, SEQ, CIGAR, RNEXT, PNEXT, TLEN) before anything is added.
int stats_add_line(const salt_index *ix, const RefIds &ids, const char *l, const char *e, uint32_t min_mapq, uint64_t *cells, uint64_t *ct)
{
    SamLine L; MRuns m; uint64_t g0 = 0;
    const int h = twin_head(ix, ids, L, "stats: ", l, e, 0, &g0);                  // (the floor is looked at below: a record below it is still mapped)
    if (h < 0) return h;
    const char *seq = L.f[9]; const size_t l_seq = L.len(9);
    if (l_seq == 0 || l_seq > 512) return L.bad("SEQ is empty or longer than 512 bases"), -1;
    int64_t pnext = 0, tlen = 0;
    if (!field_int(L.f[7], L.fe(7), &pnext) || !field_int(L.f[8], L.fe(8), &tlen) || pnext < 0 || pnext > 0x7FFFFFFF || tlen < INT32_MIN || tlen > INT32_MAX)
        return L.bad("a numeric field is no number of its range"), -1;
    const uint64_t mate = (L.flag & 0x80) ? 1 : 0;
    const bool paired = (L.flag & 1) != 0, mate_mapped = paired && !(L.flag & 8);
    int32_t rid = -1, rid_ot = -1;
    uint64_t n_i = 0, n_d = 0, n_s = 0, m_cols = 0, ops_i[64], ops_d[64]; int k_i = 0, k_d = 0;
    if (h == 1) {
        rid = ids.find(L.f[2], L.fe(2));
        if (!twin_cigar(L, g0, m)) return -1;
        if (mate_mapped) {
            if (L.is(6, '=')) rid_ot = rid;
            else if ((rid_ot = ids.find(L.f[6], L.fe(6))) < 0) return L.bad("RNEXT is no sequence of the index"), -1;
        }
        uint64_t n = 0;                                                            // (twin_cigar has checked the text: digits, then one of M I S D)
        for (const char *p = L.f[5]; p < L.fe(5); ++p) {
            if (*p >= '0' && *p <= '9') { n = 10 * n + (uint64_t)(*p - '0'); continue; }
            if (*p == 'I') { n_i += n; if (k_i < 64) ops_i[k_i++] = n; }
            else if (*p == 'D') { n_d += n; if (k_d < 64) ops_d[k_d++] = n; }
            else if (*p == 'S') n_s += n;
            n = 0;
        }
        for (int k = 0; k < m.n; ++k) {
            const uint64_t a = m.g[k], b = std::min<uint64_t>(a + m.len[k], ix->view.ref_len);
            if (a < b) m_cols += b - a;
        }
    }
    uint64_t *sn = cells + ST_SN + mate * 16;
    ++sn[0];
    uint64_t gc = 0, acgt = 0;
    for (size_t s = 0; s < l_seq; ++s) { const int b = base_code(seq[s]); if (b >= 0) ++acgt; if (b == 1 || b == 2) ++gc; }
    ++cells[ST_RL + mate * 513 + l_seq];
    ++cells[ST_GC + mate * 102 + (acgt ? (200 * gc + acgt) / (2 * acgt) : 101)];
    sn[11] += l_seq;
    if (h == 0) { ++sn[2]; return 0; }
    uint64_t *c = ct + (uint64_t)rid * 8;
    ++cells[ST_MQ + mate * 256 + (uint64_t)L.mapq];
    ++c[mate];
    if ((uint64_t)L.mapq < min_mapq) { ++sn[3]; return 0; }
    const bool rev = (L.flag & 0x10) != 0;
    ++sn[4]; ++c[2 + mate];
    if (rev) { ++sn[5]; ++c[4]; }
    if (m.gapped) ++sn[6];
    sn[12] += m_cols; c[5] += m_cols; sn[13] += n_i; sn[14] += n_d; sn[15] += n_s;
    for (int k = 0; k < k_i; ++k) ++cells[ST_ID + std::min<uint64_t>(ops_i[k], 64)];
    for (int k = 0; k < k_d; ++k) ++cells[ST_ID + 65 + std::min<uint64_t>(ops_d[k], 64)];
    uint64_t n_xa = 0;
    for (const char *t = L.nf > 11 ? L.f[11] : e; t < e; ) {
        const char *te = (const char *)memchr(t, '\t', (size_t)(e - t));
        if (!te) te = e;
        if (te - t >= 5 && memcmp(t, "XA:Z:", 5) == 0) for (const char *p = t + 5; p < te; ++p) n_xa += *p == ';';
        t = te + 1;
    }
    if (n_xa) ++sn[7];
    ++cells[ST_XA + mate * 8 + std::min<uint64_t>(n_xa, 7)];
    if (L.flag & 2) ++sn[8];
    if (!paired) return 1;
    if (!mate_mapped) { ++sn[9]; return 1; }
    if (rid_ot != rid) { ++sn[10]; return 1; }
    if (mate == 0) {
        if (tlen != 0) ++cells[ST_IS + std::min<uint64_t>((uint64_t)(tlen < 0 ? -tlen : tlen), ST_IS_MAX)];
        const bool rev_ot = (L.flag & 0x20) != 0;
        uint64_t o = 2;
        if (rev != rev_ot) o = (rev ? pnext : L.pos1) <= (rev ? L.pos1 : pnext) ? 0 : 1;
        ++cells[ST_OR + o];
    }
    return 1;
}

} // namespace

extern "C" int64_t salt_stats_add_sam(const salt_index_t *ix, const char *sam, size_t n, uint32_t min_mapq, uint64_t *cells, uint64_t n_cells, uint64_t *ct, uint64_t n_ct)
{
    if (!ix || (!sam && n) || !cells || !ct) { g_err = "stats: null argument"; return -1; }
    if (!stats_sizes(ix, n_cells, n_ct)) return -1;
    const RefIds ids(ix);
    return for_record_lines(sam, n, true, [&](const char *l, const char *e) { return stats_add_line(ix, ids, l, e, min_mapq, cells, ct); });
}

extern "C" int64_t salt_stats_text(const salt_index_t *ix, const uint64_t *cells, uint64_t n_cells, const uint64_t *ct, uint64_t n_ct, uint32_t min_mapq, char *out, uint64_t cap)
{
    if (!ix || !cells || !ct || (!out && cap)) { g_err = "stats: null argument"; return -1; }
    if (!stats_sizes(ix, n_cells, n_ct)) return -1;
    DepthOut o{ out, cap };
    static const char *const SN_KEY[16] = { "seen", "skipped", "unmapped", "low_mapq", "counted", "reverse", "gapped", "with_xa", "proper", "mate_unmapped", "mate_other_contig",
                                            "bases", "m_bases", "i_bases", "d_bases", "s_bases" };
    auto num = [&](uint64_t v) { o.put('\t'); o.putu(v); };
    const uint64_t n_mates = cells[ST_SN + 16] ? 2 : 1;                       // single end prints mate 0 only
    o.puts("#salt-stats\tv1\tmin_mapq="); o.putu(min_mapq); o.puts("\tISQ mean: hundredths, the >=4096 bin left out\n");
    for (uint64_t m = 0; m < n_mates; ++m)
        for (uint64_t k = 0; k < 16; ++k) { o.puts("SN"); num(m); o.put('\t'); o.puts(SN_KEY[k]); num(cells[ST_SN + m * 16 + k]); o.put('\n'); }
    auto hist = [&](const char *tag, uint64_t at, uint64_t width, uint64_t none) {
        for (uint64_t m = 0; m < n_mates; ++m)
            for (uint64_t k = 0; k < width; ++k) {
                const uint64_t v = cells[at + m * width + k];
                if (!v) continue;
                o.puts(tag); num(m); o.put('\t');
                if (k == none) o.puts("none"); else o.putu(k);
                num(v); o.put('\n');
            }
    };
    hist("MQ", ST_MQ, 256, ~0ull); hist("RL", ST_RL, 513, ~0ull); hist("GC", ST_GC, 102, 101); hist("XA", ST_XA, 8, ~0ull);
    const uint64_t *is = cells + ST_IS;
    auto tl = [&](uint64_t t) { o.put('\t'); if (t == ST_IS_MAX) o.puts(">=4096"); else o.putu(t); };
    uint64_t pairs = 0, in_n = 0, in_sum = 0;
    for (uint64_t t = 0; t <= ST_IS_MAX; ++t) {
        pairs += is[t];
        if (t < ST_IS_MAX) { in_n += is[t]; in_sum += t * is[t]; }
        if (is[t]) { o.puts("IS"); tl(t); num(is[t]); o.put('\n'); }
    }
    o.puts("ISQ"); num(pairs);
    for (uint64_t k = 1; k <= 3; ++k) {                                        // the smallest length at which the cumulative count reaches k quarters of the pairs
        if (!pairs) { o.puts("\t."); continue; }
        uint64_t cum = 0, t = 0;
        for (; t <= ST_IS_MAX; ++t) { cum += is[t]; if (4 * cum >= k * pairs) break; }
        tl(t);
    }
    if (!in_n) o.puts("\t.");
    else {
        // h = (100 sum + n / 2) / n without leaving 64 bits: sum = q n + r gives 100 q + (100 r + n / 2) / n
        const uint64_t hh = 100u * (in_sum / in_n) + (100u * (in_sum % in_n) + in_n / 2) / in_n;
        num(hh / 100u); o.put('.'); o.put((char)('0' + (int)(hh % 100u) / 10)); o.put((char)('0' + (int)(hh % 100u) % 10));
    }
    o.put('\n');
    o.puts("OR"); num(cells[ST_OR]); num(cells[ST_OR + 1]); num(cells[ST_OR + 2]); o.put('\n');
    for (uint64_t k = 0; k <= 64; ++k) {
        const uint64_t a = cells[ST_ID + k], b = cells[ST_ID + 65 + k];
        if (!a && !b) continue;
        o.puts("ID\t"); if (k == 64) o.puts(">=64"); else o.putu(k);
        num(a); num(b); o.put('\n');
    }
    for (size_t c = 0; c < ix->anns.size(); ++c) {
        o.puts("CT\t"); o.puts(ix->anns[c].name); num((uint64_t)ix->anns[c].len);
        for (int k = 0; k < 6; ++k) num(ct[c * 8 + (size_t)k]);
        o.put('\n');
    }
    return (int64_t)o.n;
}

// ---------------------------------------------------------------------------------------------
// Indel candidates: the host twin of k_indel_add and of the device's text kernels (salt_indel.hip; include/salt_gpu.h has the
// definition), written from that definition over this program's own SAM record lines.  It shares nothing with anything under csrc/.
// ---------------------------------------------------------------------------------------------
struct salt_indel { std::map<uint64_t, uint64_t> tab; uint64_t stat[4] = { 0, 0, 0, 0 }; };

namespace {

// letter(x) of the definition: the 2-bit genome's base, A beyond it
inline uint32_t indel_letter(const salt_index *ix, uint64_t x) { return (int64_t)x < ix->l_pac ? pac_at(ix, (uint32_t)x) : 0u; }

struct IndelOp { char what; uint64_t n, g; size_t s; };

// one record line [l, e): its M runs into diff, its I and D ops into the map and the counters; 1 it contributed, 0 it did not (unmapped,
// below min_mapq), -1 with g_err set.  The line is checked whole (head, CIGAR) before anything is added.
int indel_add_line(const salt_index *ix, const RefIds &ids, salt_indel &t, const char *l, const char *e, uint32_t min_mapq, uint32_t *diff)
{
    SamLine L; MRuns m; uint64_t g0;
    const int h = twin_head(ix, ids, L, "indels: ", l, e, min_mapq, &g0);
    if (h != 1) return h;
    if (!twin_cigar(L, g0, m)) return -1;
    const char *seq = L.f[9]; const size_t l_seq = L.len(9);
    const bool rev = (L.flag & 16) != 0;
    const uint64_t ref_len = ix->view.ref_len;
    // the ops without the soft clips (twin_cigar has checked the text: digits, then one of M I S D)
    std::vector<IndelOp> ops;
    {
        uint64_t g = g0, n = 0; size_t s = 0;
        for (const char *p = L.f[5]; p < L.fe(5); ++p) {
            if (*p >= '0' && *p <= '9') { n = 10 * n + (uint64_t)(*p - '0'); continue; }
            if (*p != 'S') ops.push_back(IndelOp{ *p, n, g, s });
            if (*p == 'M') { g += n; s += (size_t)n; } else if (*p == 'D') g += n; else s += (size_t)n;
            n = 0;
        }
    }
    for (int r = 0; r < m.n; ++r) {
        const uint64_t a = m.g[r], b = std::min<uint64_t>(a + m.len[r], ref_len);      // cut at the genome's end: not wrapped, not refused
        if (a < b) { diff[a] += 1u; diff[b] -= 1u; }
    }
    for (size_t k = 0; k < ops.size(); ++k) {
        const IndelOp &op = ops[k];
        if (op.what == 'M') continue;
        const bool del = op.what == 'D';
        const uint64_t n = op.n;
        if (n < 1 || n > (del ? SALT_INDEL_MAX_DEL : SALT_INDEL_MAX_INS)) { ++t.stat[SALT_INDEL_LONG]; continue; }
        uint64_t g = op.g;
        bool ok = k > 0 && k + 1 < ops.size() && ops[k - 1].what == 'M' && ops[k - 1].n >= 1 && ops[k + 1].what == 'M' && ops[k + 1].n >= 1 && g >= 1;
        uint64_t first = 0;
        if (ok) {
            size_t c = 0;                                                          // the last contig that begins at or in front of the anchor
            while (c + 1 < ix->anns.size() && (uint64_t)ix->anns[c + 1].offset <= g - 1) ++c;
            first = (uint64_t)ix->anns[c].offset;
            const uint64_t end = std::min<uint64_t>(c + 1 < ix->anns.size() ? (uint64_t)ix->anns[c + 1].offset : ref_len, ref_len);
            ok = g < end && (!del || g + n <= end);
        }
        uint8_t b[SALT_INDEL_MAX_INS] = { 0 };
        if (ok && !del) {
            ok = op.s + n <= l_seq;
            for (uint64_t j = 0; ok && j < n; ++j) { const int code = base_code(seq[op.s + j]); if (code < 0) ok = false; else b[j] = (uint8_t)code; }
        }
        if (!ok) { ++t.stat[SALT_INDEL_UNANCHORED]; continue; }
        for (uint32_t step = 0; step < SALT_INDEL_MAX_SHIFT && g - 1 > first; ++step) {
            const uint32_t a = indel_letter(ix, g - 1);
            if (del) { if (a != indel_letter(ix, g + n - 1)) break; }
            else {
                if (a != b[n - 1]) break;
                for (uint64_t j = n - 1; j > 0; --j) b[j] = b[j - 1];
                b[0] = (uint8_t)a;
            }
            --g;
        }
        uint64_t key = 1ull << 63 | g << 31 | (del ? 1ull << 30 : 0ull) | n << 24;
        if (!del) for (uint64_t j = 0; j < n; ++j) key |= (uint64_t)b[j] << (22 - 2 * j);
        t.tab[key] += rev ? 1ull << 32 : 1ull;
        ++t.stat[SALT_INDEL_TABLED];
    }
    return 1;
}

bool indel_sizes(const salt_index *ix, uint64_t n_pos)
{
    if (n_pos == ix->view.ref_len) return true;
    g_err = "indels: a difference array for " + std::to_string(n_pos) + " positions, the index has " + std::to_string((uint64_t)ix->view.ref_len) + " (diff: ref_len + 1 words)";
    return false;
}

} // namespace

extern "C" salt_indel_t *salt_indel_new(void) { return new salt_indel; }
extern "C" void salt_indel_free(salt_indel_t *t) { delete t; }

extern "C" int64_t salt_indel_add_sam(const salt_index_t *ix, salt_indel_t *t, const char *sam, size_t n, uint32_t min_mapq, uint32_t *diff, uint64_t n_pos)
{
    if (!ix || !t || (!sam && n) || !diff) { g_err = "indels: null argument"; return -1; }
    if (!indel_sizes(ix, n_pos)) return -1;
    const RefIds ids(ix);
    return for_record_lines(sam, n, true, [&](const char *l, const char *e) { return indel_add_line(ix, ids, *t, l, e, min_mapq, diff); });
}

extern "C" int64_t salt_indel_entries(const salt_indel_t *t, uint64_t *out, uint64_t cap)
{
    if (!t || (!out && cap)) { g_err = "indels: null argument"; return -1; }
    uint64_t n = 0;
    for (const auto &kv : t->tab) {
        if (kv.second == 0) continue;
        if (n < cap) { out[2 * n] = kv.first; out[2 * n + 1] = kv.second; }
        ++n;
    }
    return (int64_t)n;
}

extern "C" void salt_indel_stats(const salt_indel_t *t, uint64_t out[4]) { for (int i = 0; i < 4; ++i) out[i] = t ? t->stat[i] : 0; }

extern "C" int64_t salt_indel_text(const salt_index_t *ix, const uint64_t *entries, uint64_t n, const uint32_t *diff, uint64_t n_pos, uint32_t min_alt, uint32_t min_pct,
                                   char *out, uint64_t cap)
{
    if (!ix || (!entries && n) || !diff || (!out && cap)) { g_err = "indels: null argument"; return -1; }
    if (!indel_sizes(ix, n_pos)) return -1;
    if (min_alt < 1 || min_pct > 100) { g_err = "indels: min_alt is 1 .. 4294967295 and min_pct 0 .. 100"; return -1; }
    for (uint64_t i = 1; i < n; ++i) if (entries[2 * i] <= entries[2 * (i - 1)]) { g_err = "indels: the pairs are not in key order"; return -1; }
    DepthOut o{ out, cap };
    static const char NT[] = "ACGT";
    uint32_t depth = 0; uint64_t at = 0;                               // depth = the prefix sum of diff[0 .. at), mod 2^32
    size_t c = 0;                                                      // the last contig that begins at or in front of the anchor
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t key = entries[2 * i], v = entries[2 * i + 1];
        const uint64_t g = (key >> 31) & 0xFFFFFFFFull, len = (key >> 24) & 63u, bases = key & 0xFFFFFFu;
        const bool del = (key >> 30) & 1u;
        if (!(key >> 63) || g < 1 || g > n_pos || len < 1 || v == 0) continue;
        if (del ? bases != 0 : len > SALT_INDEL_MAX_INS || (bases & ((1u << (24 - 2 * len)) - 1u)) != 0) continue;
        const uint64_t a = g - 1;
        while (at <= a) depth += diff[at++];                           // (keys in order: the anchors do not go back)
        const uint64_t fwd = v & 0xFFFFFFFFull, rev = v >> 32, ao = fwd + rev;
        if (ao < min_alt || 100 * ao < (uint64_t)min_pct * depth) continue;
        while (c + 1 < ix->anns.size() && (uint64_t)ix->anns[c + 1].offset <= a) ++c;
        o.puts(ix->anns[c].name); o.put('\t'); o.putu(a - (uint64_t)ix->anns[c].offset + 1); o.puts("\t.\t");
        const char anchor = NT[indel_letter(ix, a)];
        o.put(anchor);
        if (del) for (uint64_t k = 0; k < len; ++k) o.put(NT[indel_letter(ix, g + k)]);
        o.put('\t'); o.put(anchor);
        if (!del) for (uint64_t k = 0; k < len; ++k) o.put(NT[(bases >> (22 - 2 * k)) & 3u]);
        o.puts("\t.\t.\tTYPE="); o.puts(del ? "DEL" : "INS"); o.puts(";LEN="); o.putu(len); o.puts(";DP="); o.putu(depth);
        o.puts(";AO="); o.putu(ao); o.puts(";AOF="); o.putu(fwd); o.puts(";AOR="); o.putu(rev); o.put('\n');
    }
    return (int64_t)o.n;
}

extern "C" int64_t salt_indel_header(const salt_index_t *ix, uint32_t min_mapq, uint32_t min_alt, uint32_t min_pct, uint64_t dropped, char *out, uint64_t cap)
{
    if (!ix || (!out && cap)) { g_err = "indels: null argument"; return -1; }
    DepthOut o{ out, cap };
    o.puts("##fileformat=VCFv4.2\n##source=salt --indels\n");
    for (const Ann &a : ix->anns) { o.puts("##contig=<ID="); o.puts(a.name); o.puts(",length="); o.putu((uint64_t)a.len); o.puts(">\n"); }
    o.puts("##INFO=<ID=TYPE,Number=1,Type=String,Description=\"INS or DEL\">\n"
           "##INFO=<ID=LEN,Number=1,Type=Integer,Description=\"Inserted or deleted bases\">\n"
           "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Counted reads whose M runs cover the anchor base\">\n"
           "##INFO=<ID=AO,Number=1,Type=Integer,Description=\"Counted reads that show the allele, left-normalised\">\n"
           "##INFO=<ID=AOF,Number=1,Type=Integer,Description=\"... on the forward strand\">\n"
           "##INFO=<ID=AOR,Number=1,Type=Integer,Description=\"... on the reverse strand\">\n"
           "##salt_indels_parameters=<min_mapq="); o.putu(min_mapq); o.puts(",min_alt="); o.putu(min_alt); o.puts(",min_pct="); o.putu(min_pct);
    o.puts(">\n##salt_indels_dropped="); o.putu(dropped);
    o.puts("\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n");
    return (int64_t)o.n;
}

// ---- trimming: the rule of csrc/salt_trim_rule.h on the host (include/salt_host.h) ----------------------------------------------------------
#include "../csrc/salt_trim_rule.h"

static bool trim_rule_of(const salt_trim_opt_t *o, salt::TrimRule *r)
{
    *r = salt::TrimRule();
    if (!o) return true;
    if (const char *what = salt::trim_rule_make(o->adapter, o->adapter_len, o->adapter2, o->adapter2_len, o->front, o->tail, o->qual, o->min_overlap, o->error_pct, r)) {
        g_err = what;
        return false;
    }
    return true;
}

extern "C" int salt_trim_span(const salt_trim_opt_t *opt, int mate, const char *seq, const char *qual, uint32_t len, uint32_t *beg, uint32_t *end, uint64_t *counts)
{
    if (!seq || !qual || !beg || !end || len == 0 || (mate != 0 && mate != 1)) { g_err = "trim: null argument, an empty read or a mate other than 0 and 1"; return -1; }
    salt::TrimRule r;
    if (!trim_rule_of(opt, &r)) return -1;
    salt::trim_span(r, (uint32_t)mate, reinterpret_cast<const uint8_t *>(seq), reinterpret_cast<const uint8_t *>(qual), len, beg, end,
                    counts ? counts + salt::TRIM_N_COUNTS * mate : nullptr);
    return 0;
}

extern "C" int64_t salt_trim_fastq(const salt_trim_opt_t *opt, int mate, const char *in, uint64_t n, char *out, uint64_t cap, uint64_t *counts)
{
    if ((!in && n) || (!out && cap) || (mate != 0 && mate != 1)) { g_err = "trim: null argument or a mate other than 0 and 1"; return -1; }
    salt::TrimRule r;
    if (!trim_rule_of(opt, &r)) return -1;
    uint64_t w = 0, rec = 0;
    auto put = [&](const char *p, uint64_t k) { if (w + k <= cap) memcpy(out + w, p, k); w += k; };
    auto bad = [&](const char *why) -> int64_t { g_err = "trim: input is not 4-line FASTQ at record " + std::to_string(rec) + ": " + why; return -1; };
    for (uint64_t p = 0; p < n; ++rec) {
        const char *l[4]; uint64_t len[4];
        for (int k = 0; k < 4; ++k) {
            const char *nl = p < n ? static_cast<const char *>(memchr(in + p, '\n', n - p)) : nullptr;
            if (!nl) return bad("the block does not hold whole 4-line records");
            l[k] = in + p; len[k] = (uint64_t)(nl - (in + p)); p += len[k] + 1;
            while (len[k] && l[k][len[k] - 1] == '\r') --len[k];
        }
        if (!len[0] || l[0][0] != '@') return bad("a record does not start with '@'");
        if (!len[2] || l[2][0] != '+') return bad("the third line of a record does not start with '+'");
        if (len[1] != len[3]) return bad("sequence and quality lengths differ");
        if (!len[1]) return bad("empty read");
        if (len[1] > 0xFFFFFFFFull) return bad("a read of 4 Gbases or more");
        uint32_t beg = 0, end = 0;
        salt::trim_span(r, (uint32_t)mate, reinterpret_cast<const uint8_t *>(l[1]), reinterpret_cast<const uint8_t *>(l[3]), (uint32_t)len[1], &beg, &end,
                        counts ? counts + salt::TRIM_N_COUNTS * mate : nullptr);
        put(l[0], len[0]); put("\n", 1); put(l[1] + beg, end - beg); put("\n", 1); put(l[2], len[2]); put("\n", 1); put(l[3] + beg, end - beg); put("\n", 1);
    }
    return (int64_t)w;
}

static bool trim_pair_rule_of(const salt_trim_pair_opt_t *o, salt::TrimPairRule *p)
{
    *p = salt::TrimPairRule();
    if (!o) return true;
    if (const char *what = salt::trim_pair_rule_make(o->min_overlap, o->error_pct, p)) { g_err = what; return false; }
    return true;
}

extern "C" int salt_trim_pair_span(const salt_trim_opt_t *opt, const salt_trim_pair_opt_t *pair, const char *seq1, const char *qual1, uint32_t len1,
                                   const char *seq2, const char *qual2, uint32_t len2, uint32_t span[4], uint64_t *counts, uint64_t *pair_counts)
{
    if (!seq1 || !qual1 || !seq2 || !qual2 || !span || len1 == 0 || len2 == 0) { g_err = "trim pair: null argument or an empty read"; return -1; }
    salt::TrimRule r; salt::TrimPairRule p;
    if (!trim_rule_of(opt, &r) || !trim_pair_rule_of(pair, &p)) return -1;
    salt::trim_pair_span(r, p, reinterpret_cast<const uint8_t *>(seq1), reinterpret_cast<const uint8_t *>(qual1), len1, reinterpret_cast<const uint8_t *>(seq2),
                         reinterpret_cast<const uint8_t *>(qual2), len2, span, counts, pair_counts);
    return 0;
}

// one 4-line record of in[*p, n) -> its lines without line ends; null, or what is wrong with it
static const char *trim_next_record(const char *in, uint64_t n, uint64_t *p, const char *l[4], uint64_t len[4])
{
    for (int k = 0; k < 4; ++k) {
        const char *nl = *p < n ? static_cast<const char *>(memchr(in + *p, '\n', n - *p)) : nullptr;
        if (!nl) return "the block does not hold whole 4-line records";
        l[k] = in + *p; len[k] = (uint64_t)(nl - (in + *p)); *p += len[k] + 1;
        while (len[k] && l[k][len[k] - 1] == '\r') --len[k];
    }
    if (!len[0] || l[0][0] != '@') return "a record does not start with '@'";
    if (!len[2] || l[2][0] != '+') return "the third line of a record does not start with '+'";
    if (len[1] != len[3]) return "sequence and quality lengths differ";
    if (!len[1]) return "empty read";
    if (len[1] > 0xFFFFFFFFull) return "a read of 4 Gbases or more";
    return nullptr;
}

extern "C" int salt_trim_fastq_pair(const salt_trim_opt_t *opt, const salt_trim_pair_opt_t *pair, const char *in1, uint64_t n1, const char *in2, uint64_t n2,
                                    char *out1, uint64_t cap1, uint64_t *w1, char *out2, uint64_t cap2, uint64_t *w2, uint64_t *counts, uint64_t *pair_counts)
{
    if ((!in1 && n1) || (!in2 && n2) || (!out1 && cap1) || (!out2 && cap2) || !w1 || !w2) { g_err = "trim pair: null argument"; return -1; }
    salt::TrimRule r; salt::TrimPairRule pr;
    if (!trim_rule_of(opt, &r) || !trim_pair_rule_of(pair, &pr)) return -1;
    const char *in[2] = { in1, in2 }; const uint64_t n[2] = { n1, n2 }, cap[2] = { cap1, cap2 };
    char *out[2] = { out1, out2 };
    uint64_t w[2] = { 0, 0 }, p[2] = { 0, 0 }, rec = 0;
    for (; p[0] < n1 && p[1] < n2; ++rec) {
        const char *l[2][4]; uint64_t len[2][4];
        for (int m = 0; m < 2; ++m)
            if (const char *why = trim_next_record(in[m], n[m], &p[m], l[m], len[m])) {
                g_err = "trim pair: input is not 4-line FASTQ at record " + std::to_string(rec) + " of block " + std::to_string(m + 1) + ": " + why;
                return -1;
            }
        uint32_t span[4];
        salt::trim_pair_span(r, pr, reinterpret_cast<const uint8_t *>(l[0][1]), reinterpret_cast<const uint8_t *>(l[0][3]), (uint32_t)len[0][1],
                             reinterpret_cast<const uint8_t *>(l[1][1]), reinterpret_cast<const uint8_t *>(l[1][3]), (uint32_t)len[1][1], span, counts, pair_counts);
        for (int m = 0; m < 2; ++m) {
            auto put = [&](const char *s, uint64_t k) { if (w[m] + k <= cap[m]) memcpy(out[m] + w[m], s, k); w[m] += k; };
            const uint32_t beg = span[2 * m], k = span[2 * m + 1] - beg;
            put(l[m][0], len[m][0]); put("\n", 1); put(l[m][1] + beg, k); put("\n", 1); put(l[m][2], len[m][2]); put("\n", 1); put(l[m][3] + beg, k); put("\n", 1);
        }
    }
    if (p[0] < n1 || p[1] < n2) { g_err = "trim pair: the two FASTQ blocks hold different numbers of reads"; return -1; }
    *w1 = w[0]; *w2 = w[1];
    return 0;
}
