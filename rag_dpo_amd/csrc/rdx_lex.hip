// rdx_lex.hip — the term reduction of BGE-M3's lexical weights (include/rdx.h rdx_lex_reduce; kernel: lex_kernel.hpp). The index of
// the reduced terms and its search (rdx_lex_create / _destroy / _search) share BM25's host core and live in rdx_bm25.hip.
#include "lex_kernel.hpp"
#include "rdx_host.hpp"

using namespace rdx;

extern "C" int rdx_lex_reduce(int device, const int32_t* tok, const float* w, int64_t n_tok, const int64_t* off, int64_t n_texts, int vocab,
                              const int32_t* skip_ids, int n_skip, int32_t* out_tok, uint16_t* out_w, int32_t* out_n, void* stream) {
    static const char* fn = "rdx_lex_reduce";
    if (n_texts < 0 || n_texts > INT32_MAX || n_tok < 0) return fail(RDX_ERR_INVALID, "rdx_lex_reduce: n_texts must be in [0, 2^31) and n_tok at least 0");
    if (vocab < 1) return fail(RDX_ERR_INVALID, "rdx_lex_reduce: vocab = " + std::to_string(vocab) + " must be at least 1");
    if (n_skip < 0 || n_skip > LEX_MAX_SKIP || (n_skip > 0 && !skip_ids))
        return fail(RDX_ERR_INVALID, "rdx_lex_reduce: n_skip = " + std::to_string(n_skip) + " must be in [0, " + std::to_string(LEX_MAX_SKIP) +
                                         "], with skip_ids when it is not 0");
    if (n_texts == 0) return RDX_OK;
    if (!out_n || (n_tok > 0 && (!tok || !w || !out_tok || !out_w))) return fail(RDX_ERR_INVALID, "rdx_lex_reduce: null pointer");
    if ((((uintptr_t)tok | (uintptr_t)w | (uintptr_t)out_tok | (uintptr_t)out_n) & 3) || ((uintptr_t)out_w & 1))
        return fail(RDX_ERR_INVALID, "rdx_lex_reduce: misaligned pointer");
    RDX_TRY(check_device_index(fn, device));
    HIP_TRY(hipSetDevice(device));
    const void* d_off;
    RDX_TRY(shape_array(fn, "off", off, 8, &d_off));
    if (off[0] < 0) return fail(RDX_ERR_INVALID, "rdx_lex_reduce: off must start at 0 or above");
    int64_t longest = 0;
    for (int64_t i = 0; i < n_texts; ++i) {
        const int64_t n = off[i + 1] - off[i];
        if (n < 0 || n > LEX_MAX_TOKENS)
            return fail(RDX_ERR_INVALID, "rdx_lex_reduce: text " + std::to_string(i) + " has " + std::to_string(n) + " tokens (0.." +
                                             std::to_string(LEX_MAX_TOKENS) + "; off must not decrease)");
        longest = std::max(longest, n);
    }
    if (off[n_texts] > n_tok)
        return fail(RDX_ERR_INVALID, "rdx_lex_reduce: off ends at " + std::to_string(off[n_texts]) + ", behind n_tok = " + std::to_string(n_tok));
    LexSkip skip{};
    skip.n = n_skip;
    for (int s = 0; s < n_skip; ++s) skip.id[s] = skip_ids[s];
    const int key_cap = lex_pow2_at_least((int)std::max<int64_t>(longest, 1));
    const size_t lds = lex_lds_bytes((int)longest);
    RDX_TRY(dynamic_lds(device, reinterpret_cast<const void*>(k_lex_reduce), lds));
    const int threads = longest > 1024 ? LEX_THREADS : LEX_THREADS_SMALL;
    hipLaunchKernelGGL(k_lex_reduce, dim3((unsigned)n_texts), dim3(threads), lds, (hipStream_t)stream, tok, w, (const int64_t*)d_off, n_tok,
                       vocab, skip, key_cap, out_tok, out_w, out_n);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}
