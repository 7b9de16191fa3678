// tools/inflate_model.cc -- the device's BGZF member decoder (salt_amd/csrc/salt_inflate_block.h) run on the host, one thread of the
// workgroup after the other:  inflate_model < text.gz > text   (any number of BGZF members; exit 3 and "block N: reason" on stderr when
// one is bad).  It is where the decoder's bounds rules are proven (tests/test_inflate_model.py builds it with AddressSanitizer and feeds it
// damaged members) and what the tests' stand-in for the device library inflates with; salt never runs it.
//   g++ -O2 -std=c++17 -o inflate_model tools/inflate_model.cc
#include "../salt_amd/csrc/salt_inflate_block.h"
#include <cstdio>
#include <memory>
#include <vector>

int main()
{
    using namespace salt::bgzf;
    std::vector<uint8_t> in;
    { uint8_t buf[1 << 16]; size_t r; while ((r = fread(buf, 1, sizeof buf, stdin)) > 0) in.insert(in.end(), buf, buf + r); }
    auto lds = std::make_unique<InflateLds>();
    size_t n_blocks = 0, text = 0;
    for (size_t at = 0; at < in.size(); ++n_blocks) {
        const uint8_t *h = in.data() + at;
        const size_t left = in.size() - at;
        uint32_t status = INFL_E_HEADER, csize = 0, usize = 0;
        if (left >= 18 && h[0] == 0x1f && h[1] == 0x8b && h[12] == 'B' && h[13] == 'C') {         // (the decoder reads the extra field properly: this only finds the member's end)
            csize = (h[16] | h[17] << 8) + 1u;
            status = csize < 26 || csize > left ? INFL_E_BSIZE : INFL_OK;
        }
        if (status == INFL_OK) {
            const uint8_t *t = h + csize - 4;
            usize = t[0] | t[1] << 8 | t[2] << 16 | (uint32_t)t[3] << 24;
            // the member and its text in allocations of exactly their sizes (behind a few bytes that shift their alignment): a read or
            // write past either end is the sanitizer's to see
            const size_t shift = n_blocks & 3;
            std::vector<uint8_t> member(shift + csize), out(shift + (usize <= INFL_MAX ? usize : 0), 0xAA);
            memcpy(member.data() + shift, h, csize);
            status = 0xDEADBEEFu;
            inflate_block(*lds, member.data() + shift, csize, out.data() + shift, usize, &status, 0);
            if (status == INFL_OK && usize) { fwrite(out.data() + shift, 1, usize, stdout); text += usize; }
        }
        if (status != INFL_OK) { fprintf(stderr, "block %zu: %s\n", n_blocks, inflate_reason(status)); return 3; }
        at += csize;
    }
    fprintf(stderr, "%zu blocks, %zu -> %zu bytes\n", n_blocks, in.size(), text);
    return fflush(stdout) == 0 ? 0 : 1;
}
