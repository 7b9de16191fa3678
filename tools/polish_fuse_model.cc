// tools/polish_fuse_model.cc -- the record-to-hits rule of `salt --polish` (pl_row_hits, salt_amd/csrc/salt_polish_text.h: the source
// k_pl_rows of salt_polish.hip compiles) held against the route it replaces, on the host.  Stand-alone: g++ -std=c++17, with or without
// -fsanitize=address,undefined (tests/test_salt_polish_model.py builds it with them and runs it directly).
//
//   polish_fuse_model [-p] <index>.C.ann <rows.bin> <lines.sam>
//
// rows.bin: result rows (salt_result_t, 880 bytes each); lines.sam: the SAM line made from each row, one line a row, in order (an empty
// line: a skipped read).  Per row, the hits pl_row_hits + pl_sort_unique take from the row against the hits pl_parse + pl_hits +
// pl_sort_unique take from the line: the lists of (strand, offset, pos, contig name) must be equal, and so must bit 0x10 of FLAG
// (pl_row_rev).  The row side sees the contig table in the index's order, as the fused route does; the line side the name-sorted table
// of the text route.  -p: the rows are mates of pairs.
// Prints one "D <row> ..." line per difference and a summary; exit status 1 when anything differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>
#include "../include/salt_gpu.h"
#include "../salt_amd/csrc/salt_polish_text.h"

using namespace salt_pl;

static bool slurp(const char *path, std::vector<uint8_t> &v)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return true;
}

struct Hit { uint32_t strand, offset, pos; std::string contig; };
static bool same(const Hit &a, const Hit &b) { return a.strand == b.strand && a.offset == b.offset && a.pos == b.pos && a.contig == b.contig; }
static std::string show(const std::vector<Hit> &v)
{
    std::string s;
    for (const Hit &h : v) s += " (" + std::to_string(h.strand) + "," + std::to_string(h.offset) + "," + h.contig + "," + std::to_string(h.pos) + ")";
    return s.empty() ? " -" : s;
}

int main(int argc, char **argv)
{
    bool paired = false;
    int a = 1;
    if (a < argc && !strcmp(argv[a], "-p")) { paired = true; ++a; }
    if (argc - a != 3) { fprintf(stderr, "usage: polish_fuse_model [-p] <index>.C.ann <rows.bin> <lines.sam>\n"); return 2; }
    FILE *fa = fopen(argv[a], "r");
    if (!fa) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
    long long l_pac = 0; int n_seqs = 0; unsigned seed = 0;
    if (fscanf(fa, "%lld%d%u", &l_pac, &n_seqs, &seed) != 3 || n_seqs < 1) { fprintf(stderr, "%s: bad first line\n", argv[a]); return 2; }
    std::vector<std::pair<std::string, int64_t>> tab;
    for (int i = 0; i < n_seqs; ++i) {
        unsigned gi; char name[1024], anno[4096]; long long off; int len, amb;
        if (fscanf(fa, "%u%1023s", &gi, name) != 2 || !fgets(anno, sizeof anno, fa) || fscanf(fa, "%lld%d%d", &off, &len, &amb) != 3) { fprintf(stderr, "%s: bad record %d\n", argv[a], i); return 2; }
        tab.push_back({ name, off });
    }
    fclose(fa);
    // the index's order (row side), exactly n_seqs offsets: a search that leaves the table is a sanitizer report
    std::vector<int64_t> ix_off;
    for (auto &t : tab) ix_off.push_back(t.second);
    const std::vector<std::pair<std::string, int64_t>> ix_tab = tab;
    // sorted by name (line side)
    std::stable_sort(tab.begin(), tab.end(), [](const std::pair<std::string, int64_t> &x, const std::pair<std::string, int64_t> &y) { return x.first < y.first; });
    std::vector<int64_t> c_off; std::vector<uint32_t> name_off; std::vector<uint8_t> names;
    for (auto &t : tab) { name_off.push_back((uint32_t)names.size()); names.insert(names.end(), t.first.begin(), t.first.end()); c_off.push_back(t.second); }
    name_off.push_back((uint32_t)names.size());
    names.push_back(0);
    PlContigs ct; ct.off = c_off.data(); ct.name_off = name_off.data(); ct.names = names.data(); ct.n = (int32_t)c_off.size();

    std::vector<uint8_t> rows_raw, text;
    if (!slurp(argv[a + 1], rows_raw) || rows_raw.size() % sizeof(salt_result_t)) { fprintf(stderr, "%s: not whole result rows\n", argv[a + 1]); return 2; }
    if (!slurp(argv[a + 2], text)) { fprintf(stderr, "cannot read %s\n", argv[a + 2]); return 2; }
    const size_t n_rows = rows_raw.size() / sizeof(salt_result_t);
    std::vector<salt_result_t> rows(n_rows);
    if (n_rows) memcpy(rows.data(), rows_raw.data(), rows_raw.size());
    const uint8_t *s = text.data();
    const uint32_t n = (uint32_t)text.size();
    uint32_t p = 0;
    size_t n_diff = 0, n_hits = 0, n_empty = 0, row = 0;
    for (; row < n_rows; ++row) {
        if (p >= n) { printf("D %zu no line for this row\n", row); ++n_diff; break; }
        uint32_t e = p;
        while (e < n && s[e] != '\n') ++e;
        const salt_result_t &q = rows[row];
        std::vector<Hit> from_row, from_line;
        bool line_ok = true, rev_line = false;
        const bool rev_row = pl_row_rev(q, paired);
        if (e == p) {                                            // a skipped read's empty line: no record on either route
            ++n_empty;
            if (!q.skipped) { printf("D %zu an empty line for a row that is not skipped\n", row); ++n_diff; }
            p = e + 1;
            continue;
        }
        if (q.skipped && !paired) { printf("D %zu a line for a skipped row\n", row); ++n_diff; }
        {   // the row
            PlHit h[2][PL_ROW_HITS]; uint32_t nh[2];              // exactly the spans k_pl_rows gives a record
            pl_row_hits(q, paired, ix_off.data(), (int32_t)ix_off.size(), h[0], h[1], nh);
            for (uint32_t st = 0; st < 2; ++st) {
                const uint32_t nu = pl_sort_unique(h[st], nh[st]);
                for (uint32_t j = 0; j < nu; ++j) from_row.push_back(Hit{ st, h[st][j].offset, h[st][j].pos, ix_tab[h[st][j].contig].first });
            }
        }
        {   // the line
            PlFields f; uint32_t nh[2] = { 0, 0 }, bb = 0, be = 0;
            if (!pl_parse(s, p, e, f)) line_ok = false;
            else {
                rev_line = (f.flag & 0x10) != 0;
                pl_hits(s, f, ct, false, (PlHit *)nullptr, (PlHit *)nullptr, nh, bb, be);
                std::vector<PlHit> hits((size_t)nh[0] + nh[1]);
                uint32_t nh2[2];
                PlHit *h0 = hits.data(), *h1 = hits.data() + nh[0];
                if (!pl_hits(s, f, ct, true, h0, h1, nh2, bb, be)) line_ok = false;
                else
                    for (uint32_t st = 0; st < 2; ++st) {
                        PlHit *h = st ? h1 : h0;
                        const uint32_t nu = pl_sort_unique(h, nh[st]);
                        for (uint32_t j = 0; j < nu; ++j)
                            from_line.push_back(Hit{ st, h[j].offset, h[j].pos, std::string((const char *)names.data() + name_off[h[j].contig], name_off[h[j].contig + 1] - name_off[h[j].contig]) });
                    }
            }
        }
        bool eq = line_ok && from_row.size() == from_line.size() && rev_row == rev_line;
        for (size_t j = 0; eq && j < from_row.size(); ++j) eq = same(from_row[j], from_line[j]);
        if (!eq) {
            printf("D %zu row: 0x10 %d%s line: 0x10 %d%s%s\n", row, (int)rev_row, show(from_row).c_str(), (int)rev_line, show(from_line).c_str(), line_ok ? "" : " (the line does not parse)");
            ++n_diff;
        }
        n_hits += from_row.size();
        p = e + 1;
    }
    if (row == n_rows && p < n) { printf("D %zu lines behind the last row\n", n_rows); ++n_diff; }
    printf("rows %zu empty %zu hits %zu differences %zu\n", n_rows, n_empty, n_hits, n_diff);
    return n_diff ? 1 : 0;
}
