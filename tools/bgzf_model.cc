// tools/bgzf_model.cc -- the device's BGZF block algorithm (salt_amd/csrc/salt_bgzf_block.h) run on the host, one thread of the workgroup
// after the other:  bgzf_model < text > text.gz   (no end-of-file block; stderr: blocks, text bytes, file bytes, stored blocks).
// It is a check of the phase list (tests/test_bgzf_model.py inflates what it writes) and a way to try a block cut or a hash width
// without a GPU; salt never runs it.
//   g++ -O2 -std=c++17 -o bgzf_model tools/bgzf_model.cc
#include "../salt_amd/csrc/salt_bgzf_block.h"
#include <cstdio>
#include <memory>
#include <vector>

int main()
{
    using namespace salt::bgzf;
    std::vector<uint8_t> in;
    { uint8_t buf[1 << 16]; size_t r; while ((r = fread(buf, 1, sizeof buf, stdin)) > 0) in.insert(in.end(), buf, buf + r); }
    const size_t n = in.size();
    in.resize(n + 64, 0xAA);                                  // what lies behind the text must not matter
    auto lds = std::make_unique<BlockLds>();
    std::vector<uint32_t> slot(BGZF_SLOT / 4);
    size_t out_bytes = 0, n_stored = 0, n_blocks = 0;
    for (size_t at = 0; at < n; at += BGZF_CUT, ++n_blocks) {
        const uint32_t len = (uint32_t)(n - at < BGZF_CUT ? n - at : BGZF_CUT);
        uint32_t size = 0;
        std::fill(slot.begin(), slot.end(), 0xDEADBEEFu);     // nor what the slot held before
        deflate_block(*lds, in.data() + at, len, slot.data(), &size, 0);
        n_stored += lds->stored;
        fwrite(slot.data(), 1, size, stdout);
        out_bytes += size;
    }
    fprintf(stderr, "%zu blocks, %zu -> %zu bytes, %zu stored\n", n_blocks, n, out_bytes, n_stored);
    return 0;
}
