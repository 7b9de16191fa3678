// tests/stub/salt_gpu_inflate_stub.cc -- TEST INFRASTRUCTURE: the three workspace entry points of the device inflate path for the stand-in
// library of salt_gpu_stub.c (linked together with it, which stays as it is): "the device's text buffer" is a string per workspace, the
// members are inflated by the host model of the kernel's own source (salt_amd/csrc/salt_inflate_block.h), and the align call hands the range
// to that stub's salt_gpu_align_se_text.  With it the `salt` binary takes its device-inflate path without a GPU (tests/test_inflate_cli_stub.py).
#include "../../include/salt_gpu.h"
#include "../../salt_amd/csrc/salt_inflate_block.h"
#include <map>
#include <memory>
#include <mutex>
#include <string>

static std::mutex g_mu;
static std::map<salt_gpu_ws_t *, std::string> g_text;          // never erased: a workspace created at a destroyed one's address starts by inflating

static std::string *text_of(salt_gpu_ws_t *ws) { std::lock_guard<std::mutex> lk(g_mu); return &g_text[ws]; }

extern "C" int salt_gpu_ws_inflate_bgzf(salt_gpu_ws_t *ws, const void *blocks, uint64_t n_cbytes, uint32_t n_blocks, const uint32_t *c_off, const uint32_t *u_off)
{
    using namespace salt::bgzf;
    std::string &text = *text_of(ws);
    text.clear();
    if (n_blocks == 0) return SALT_OK;
    if (c_off[n_blocks] > n_cbytes) return SALT_E_INVAL;
    std::string out(u_off[n_blocks], '\xAA');
    auto lds = std::make_unique<InflateLds>();
    for (uint32_t b = 0; b < n_blocks; ++b) {
        uint32_t status = 0xDEADBEEFu;
        inflate_block(*lds, static_cast<const uint8_t *>(blocks) + c_off[b], c_off[b + 1] - c_off[b], reinterpret_cast<uint8_t *>(&out[0]) + u_off[b], u_off[b + 1] - u_off[b], &status, 0);
        if (status != INFL_OK) return SALT_E_DATA;
    }
    text.swap(out);
    return SALT_OK;
}

extern "C" int salt_gpu_ws_text_peek(salt_gpu_ws_t *ws, uint64_t off, uint64_t n, void *dst)
{
    const std::string &text = *text_of(ws);
    if (off > text.size() || n > text.size() - off) return SALT_E_INVAL;
    if (n) memcpy(dst, text.data() + off, n);
    return SALT_OK;
}

extern "C" int salt_gpu_align_se_text_dev(salt_gpu_ws_t *ws, const salt_aln_opt_t *opt, const salt_text_opt_t *topt, uint64_t off, uint64_t n_bytes, int add_newline,
                                          const char **sam, uint64_t *sam_bytes, uint32_t *n_reads)
{
    const std::string &text = *text_of(ws);
    *sam = nullptr; *sam_bytes = 0; *n_reads = 0;
    if (off > text.size() || n_bytes > text.size() - off) return SALT_E_INVAL;
    std::string block = text.substr(off, n_bytes);
    if (add_newline) block.push_back('\n');
    return salt_gpu_align_se_text(ws, opt, topt, block.data(), block.size(), sam, sam_bytes, n_reads);
}
