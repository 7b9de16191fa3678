// tools/polish_text_model.cc -- the per-record rules of `polish` over SAM text (salt_amd/csrc/salt_polish_text.h: the source the device
// kernels of salt_polish.hip compile) run on the host, one record after the other.  Stand-alone: g++ -std=c++17, with or without
// -fsanitize=address,undefined (tests/test_polish_text_model.py builds both and feeds them the fixtures and damaged records).
//
//   polish_text_model [-s] [-k] <index>.C.ann <index>.C.pac <records.sam>
//
// Header lines are skipped, an empty line ends the input.  Per record it prints
//   R <index> flag <flag> l_seq <n> hits <parsed forward> <parsed reverse> unique <forward> <reverse>
//   H <strand> <offset> <contig> <pos>                         the unique hits in offset order, forward strand first
//   I <offset> <tlen> <strand> <pool: 0 / 1> <window>          one per unique hit; window: the l_seq codes of an explicit pool window, else -
// and stops at the first record with a status: "status <code> record <index>" on the last line, exit status 3.  With -k it keeps going
// behind such a record (the exit status is still 3): a file of damaged records, one a line, is one run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>
#include "../salt_amd/csrc/salt_polish_text.h"

using namespace salt_pl;

struct Item { uint32_t read, offset, pool; uint16_t tlen; uint8_t strand, k; };    // salt_polish_item_t

static bool slurp(const char *path, std::vector<uint8_t> &v)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    bool use_sw = false, keep = false;
    int a = 1, rc = 0;
    for (; a < argc && argv[a][0] == '-'; ++a) { if (!strcmp(argv[a], "-s")) use_sw = true; else if (!strcmp(argv[a], "-k")) keep = true; else break; }
    if (argc - a != 3) { fprintf(stderr, "usage: polish_text_model [-s] [-k] <index>.C.ann <index>.C.pac <records.sam>\n"); return 2; }
    // the contig table (bntann1_t: offset + name), sorted by name
    FILE *fa = fopen(argv[a], "r");
    if (!fa) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
    long long l_pac = 0; int n_seqs = 0; unsigned seed = 0;
    if (fscanf(fa, "%lld%d%u", &l_pac, &n_seqs, &seed) != 3) { fprintf(stderr, "%s: bad first line\n", argv[a]); return 2; }
    std::vector<std::pair<std::string, int64_t>> tab;
    for (int i = 0; i < n_seqs; ++i) {
        unsigned gi; char name[1024], anno[4096]; long long off; int len, amb;
        if (fscanf(fa, "%u%1023s", &gi, name) != 2 || !fgets(anno, sizeof anno, fa) || fscanf(fa, "%lld%d%d", &off, &len, &amb) != 3) { fprintf(stderr, "%s: bad record %d\n", argv[a], i); return 2; }
        tab.push_back({ name, off });
    }
    fclose(fa);
    std::stable_sort(tab.begin(), tab.end(), [](const std::pair<std::string, int64_t> &x, const std::pair<std::string, int64_t> &y) { return x.first < y.first; });
    std::vector<int64_t> c_off; std::vector<uint32_t> name_off; std::vector<uint8_t> names;
    for (auto &t : tab) { name_off.push_back((uint32_t)names.size()); names.insert(names.end(), t.first.begin(), t.first.end()); c_off.push_back(t.second); }
    name_off.push_back((uint32_t)names.size());
    names.push_back(0);
    PlContigs ct; ct.off = c_off.data(); ct.name_off = name_off.data(); ct.names = names.data(); ct.n = (int32_t)c_off.size();
    std::vector<uint8_t> pac, text;
    if (!slurp(argv[a + 1], pac) || pac.size() < (size_t)l_pac / 4 + 1) { fprintf(stderr, "cannot read %s\n", argv[a + 1]); return 2; }
    if (!slurp(argv[a + 2], text)) { fprintf(stderr, "cannot read %s\n", argv[a + 2]); return 2; }
    // an exact copy, so that a read one byte past the text is a sanitizer report
    std::vector<uint8_t> exact(text.begin(), text.end());
    const uint8_t *s = exact.data();
    const uint32_t n = (uint32_t)exact.size();
    uint32_t p = 0, recno = 0;
    bool in_header = true;
    while (p < n) {
        uint32_t e = p;
        while (e < n && s[e] != '\n') ++e;
        if (in_header && s[p] == '@') { p = e + 1; continue; }
        in_header = false;
        if (e == p) break;                                      // an empty line ends the input
        PlFields f;
        int status = PL_OK;
        uint32_t nh[2] = { 0, 0 }, nu[2] = { 0, 0 }, bb = 0, be = 0, n_clip = 0;
        std::vector<PlHit> hits; std::vector<Item> items; std::vector<uint8_t> pool;
        if (!pl_parse(s, p, e, f)) status = PL_E_FIELDS;
        else if (f.l_seq == 0 || f.l_seq > PL_MAX_READ) status = PL_E_LEN;
        else {
            pl_hits(s, f, ct, false, (PlHit *)nullptr, (PlHit *)nullptr, nh, bb, be);       // the count pass
            hits.resize((size_t)nh[0] + nh[1]);                  // exactly: a fill pass that disagrees writes out of bounds
            uint32_t nh2[2];
            PlHit *h0 = hits.data(), *h1 = hits.data() + nh[0];
            if (!pl_hits(s, f, ct, true, h0, h1, nh2, bb, be)) status = PL_E_CONTIG;
            else {
                nu[0] = pl_sort_unique(h0, nh[0]); nu[1] = pl_sort_unique(h1, nh[1]);
                status = pl_windows<Item>(recno, f.l_seq, (uint64_t)l_pac, use_sw, h0, nu[0], h1, nu[1], pac.data(), nullptr, nullptr, 0, n_clip);
                if (!status) {
                    items.resize((size_t)nu[0] + nu[1]); pool.resize((size_t)(use_sw ? 0 : n_clip) * PL_POOL_STRIDE);
                    uint32_t n_clip2 = 0;
                    pl_windows<Item>(recno, f.l_seq, (uint64_t)l_pac, use_sw, h0, nu[0], h1, nu[1], pac.data(), items.data(), pool.data(), 0, n_clip2);
                }
            }
        }
        if (status) {
            printf("status %d record %u\n", status, recno);
            if (!keep) return 3;
            rc = 3; ++recno; p = e + 1;
            continue;
        }
        std::vector<uint8_t> codes(f.l_seq);
        pl_codes(s, f, codes.data());
        printf("R %u flag %d l_seq %u hits %u %u unique %u %u codes ", recno, f.flag, f.l_seq, nh[0], nh[1], nu[0], nu[1]);
        for (uint8_t c : codes) putchar('0' + c);
        putchar('\n');
        for (uint32_t st = 0; st < 2; ++st)
            for (uint32_t j = 0; j < nu[st]; ++j) {
                const PlHit &x = hits[(st ? nh[0] : 0) + j];
                printf("H %u %u %.*s %u\n", st, x.offset, (int)(name_off[x.contig + 1] - name_off[x.contig]), (const char *)names.data() + name_off[x.contig], x.pos);
            }
        for (const Item &x : items) {
            printf("I %u %u %u %d ", x.offset, (unsigned)x.tlen, (unsigned)x.strand, x.pool != 0xFFFFFFFFu);
            if (x.pool == 0xFFFFFFFFu) putchar('-');
            else for (uint32_t i = 0; i < f.l_seq; ++i) putchar('0' + pool[(size_t)x.pool * PL_POOL_STRIDE + i]);
            putchar('\n');
        }
        ++recno;
        p = e + 1;
    }
    return rc;
}
