// rdx_enc.hip — the encoder launchers (rdx_enc_*), the reranker head and selection (rdx_rerank_*) and the topic boost
// (rdx_topic_boost) of include/rdx.h, and their forms for a batch of questions (rdx_rerank_head_rows_f16, rdx_topic_boost_batch,
// rdx_rerank_select_batch).
#include "rdx_host.hpp"

#include "enc_kernels.hpp"
#include "enc_small.hpp"
#include "enc_gemm.hpp"
#include "rerank_kernel.hpp"
#include "topic_kernel.hpp"
#include "rerank_batch_kernel.hpp"

using namespace rdx;

extern "C" int rdx_enc_attention_f16(int device, const void* qkv, const int32_t* tok_first, const int32_t* tok_len, int64_t n_tokens,
                                     int heads, int head_dim, float scale, int max_text_tokens, void* ctx, void* stream) {
    if (n_tokens < 0 || heads < 1 || heads > 65535) return fail(RDX_ERR_INVALID, "rdx_enc_attention_f16: bad shape");
    if (head_dim != ENC_HEAD_DIM) return fail(RDX_ERR_INVALID, "rdx_enc_attention_f16: head_dim must be 64");
    if (n_tokens == 0) return RDX_OK;
    if (!qkv || !tok_first || !tok_len || !ctx) return fail(RDX_ERR_INVALID, "rdx_enc_attention_f16: null pointer");
    if (((uintptr_t)qkv | (uintptr_t)ctx) & 15) return fail(RDX_ERR_INVALID, "rdx_enc_attention_f16: qkv and ctx must be 16-byte aligned");
    RDX_TRY(check_device_index("rdx_enc_attention_f16", device));
    HIP_TRY(hipSetDevice(device));
    // keys a workgroup stages in LDS: its 64 tokens' texts span at most 64 + 2 (L - 1) tokens when no text is longer than L
    int window = ENC_KEY_WINDOW;
    if (max_text_tokens > 0) window = std::min<int64_t>(ENC_KEY_WINDOW, (64 + 2 * ((int64_t)max_text_tokens - 1) + 7) / 8 * 8);
    hipLaunchKernelGGL(k_enc_attention, dim3((unsigned)((n_tokens + 63) / 64), (unsigned)heads), dim3(256), (size_t)window * 256, (hipStream_t)stream,
                       (const _Float16*)qkv, tok_first, tok_len, n_tokens, heads, scale, window, (_Float16*)ctx);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_enc_attention_mfma_f16(int device, const void* qkv, const int32_t* query_blocks, int n_blocks, int heads, int head_dim,
                                          float scale, void* ctx, void* stream) {
    if (n_blocks < 0 || heads < 1 || heads > 65535) return fail(RDX_ERR_INVALID, "rdx_enc_attention_mfma_f16: bad shape");
    if (head_dim != ENC_HEAD_DIM) return fail(RDX_ERR_INVALID, "rdx_enc_attention_mfma_f16: head_dim must be 64");
    if (n_blocks == 0) return RDX_OK;
    if (!qkv || !query_blocks || !ctx) return fail(RDX_ERR_INVALID, "rdx_enc_attention_mfma_f16: null pointer");
    if (((uintptr_t)qkv | (uintptr_t)ctx | (uintptr_t)query_blocks) & 15) return fail(RDX_ERR_INVALID, "rdx_enc_attention_mfma_f16: pointers must be 16-byte aligned");
    RDX_TRY(check_device_index("rdx_enc_attention_mfma_f16", device));
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(k_enc_attention_mfma, dim3((unsigned)n_blocks, (unsigned)heads), dim3(256), 0, (hipStream_t)stream, (const _Float16*)qkv, query_blocks, heads,
                       scale * 1.4426950408889634f, (_Float16*)ctx);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

template <bool GELU>
static void launch_linear_small(int ntb, dim3 grid, hipStream_t st, const _Float16* x, const _Float16* w, const _Float16* b, int T, int N, int K,
                                _Float16* out) {
    if (ntb <= 2 && K % 1024 == 0 && K <= 4096) {   // one question: 16 waves split K, a wave's whole slice in flight at once
        const size_t lds = (size_t)16 * ntb * 1024;
        if (ntb == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_linear_small<1, GELU, 16>), grid, dim3(1024), lds, st, x, w, b, T, N, K, out);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_linear_small<2, GELU, 16>), grid, dim3(1024), lds, st, x, w, b, T, N, K, out);
        return;
    }
    const size_t lds = (size_t)ntb * 4096;   // 4 waves x ntb * 4 registers x 64 lanes x 4 B
    switch (ntb) {
        case 1: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_linear_small<1, GELU, 4>), grid, dim3(256), lds, st, x, w, b, T, N, K, out); break;
        case 2: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_linear_small<2, GELU, 4>), grid, dim3(256), lds, st, x, w, b, T, N, K, out); break;
        case 4: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_linear_small<4, GELU, 4>), grid, dim3(256), lds, st, x, w, b, T, N, K, out); break;
        case 8: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_linear_small<8, GELU, 4>), grid, dim3(256), lds, st, x, w, b, T, N, K, out); break;
        default: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_linear_small<16, GELU, 4>), grid, dim3(256), lds, st, x, w, b, T, N, K, out); break;
    }
}

extern "C" int rdx_enc_linear_small_f16(int device, const void* x, const void* w, const void* bias, int n_tokens, int n_out, int n_in,
                                        int act, void* out, void* stream) {
    if (n_tokens < 0 || n_tokens > 256) return fail(RDX_ERR_INVALID, "rdx_enc_linear_small_f16: at most 256 tokens (use the BLAS library beyond)");
    if (n_out < 16 || n_out % 16 || n_in < 512 || n_in % 512) return fail(RDX_ERR_INVALID, "rdx_enc_linear_small_f16: n_out must be a multiple of 16, n_in of 512");
    if (act != 0 && act != 1) return fail(RDX_ERR_INVALID, "rdx_enc_linear_small_f16: act is 0 (none) or 1 (erf GELU)");
    if (n_tokens == 0) return RDX_OK;
    if (!x || !w || !bias || !out) return fail(RDX_ERR_INVALID, "rdx_enc_linear_small_f16: null pointer");
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)out) & 15) return fail(RDX_ERR_INVALID, "rdx_enc_linear_small_f16: x, w and out must be 16-byte aligned");
    RDX_TRY(check_device_index("rdx_enc_linear_small_f16", device));
    HIP_TRY(hipSetDevice(device));
    int ntb = 1;
    while (ntb * 16 < n_tokens) ntb *= 2;
    const dim3 grid((unsigned)(n_out / 16));
    if (act) launch_linear_small<true>(ntb, grid, (hipStream_t)stream, (const _Float16*)x, (const _Float16*)w, (const _Float16*)bias, n_tokens, n_out, n_in, (_Float16*)out);
    else launch_linear_small<false>(ntb, grid, (hipStream_t)stream, (const _Float16*)x, (const _Float16*)w, (const _Float16*)bias, n_tokens, n_out, n_in, (_Float16*)out);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_enc_add_layernorm_f16(int device, const void* a, const void* b, const void* gamma, const void* beta, float eps,
                                         int64_t rows, int hidden, void* out, void* stream) {
    if (rows < 0 || hidden < 512 || hidden > 2048 || hidden % 512) return fail(RDX_ERR_INVALID, "rdx_enc_add_layernorm_f16: hidden must be 512, 1024, 1536 or 2048");
    if (rows == 0) return RDX_OK;
    if (!a || !b || !gamma || !beta || !out) return fail(RDX_ERR_INVALID, "rdx_enc_add_layernorm_f16: null pointer");
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15)
        return fail(RDX_ERR_INVALID, "rdx_enc_add_layernorm_f16: pointers must be 16-byte aligned");
    RDX_TRY(check_device_index("rdx_enc_add_layernorm_f16", device));
    HIP_TRY(hipSetDevice(device));
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const _Float16 *pa = (const _Float16*)a, *pb = (const _Float16*)b, *pg = (const _Float16*)gamma, *pbt = (const _Float16*)beta;
    switch (hidden / 512) {
        case 1: hipLaunchKernelGGL(k_enc_add_ln<1>, grid, block, 0, st, pa, pb, pg, pbt, eps, rows, (_Float16*)out); break;
        case 2: hipLaunchKernelGGL(k_enc_add_ln<2>, grid, block, 0, st, pa, pb, pg, pbt, eps, rows, (_Float16*)out); break;
        case 3: hipLaunchKernelGGL(k_enc_add_ln<3>, grid, block, 0, st, pa, pb, pg, pbt, eps, rows, (_Float16*)out); break;
        default: hipLaunchKernelGGL(k_enc_add_ln<4>, grid, block, 0, st, pa, pb, pg, pbt, eps, rows, (_Float16*)out); break;
    }
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

constexpr int64_t ENC_MAX_WORKGROUPS = (1 << 24) - 1;   // x 256 threads < 2^32, the most one launch holds

extern "C" int rdx_enc_layernorm_f16(int device, const void* s, const void* gamma, const void* beta, float eps, int64_t rows, int hidden,
                                     void* out, void* stream) {
    if (hidden < 512 || hidden > 2048 || hidden % 512) return fail(RDX_ERR_INVALID, "rdx_enc_layernorm_f16: hidden must be 512, 1024, 1536 or 2048");
    // one workgroup of 256 threads per 4 rows; a launch holds fewer than 2^32 threads
    if (rows < 0 || (rows + 3) / 4 > ENC_MAX_WORKGROUPS) return fail(RDX_ERR_INVALID, "rdx_enc_layernorm_f16: rows must be in [0, 4 * (2^24 - 1)]");
    if (rows == 0) return RDX_OK;
    if (!s || !gamma || !beta || !out) return fail(RDX_ERR_INVALID, "rdx_enc_layernorm_f16: null pointer");
    if (((uintptr_t)s | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15)
        return fail(RDX_ERR_INVALID, "rdx_enc_layernorm_f16: pointers must be 16-byte aligned");
    RDX_TRY(check_device_index("rdx_enc_layernorm_f16", device));
    HIP_TRY(hipSetDevice(device));
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const _Float16 *ps = (const _Float16*)s, *pg = (const _Float16*)gamma, *pbt = (const _Float16*)beta;
    switch (hidden / 512) {   // the add + LayerNorm kernel without its second operand
        case 1: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_add_ln<1, false>), grid, block, 0, st, ps, ps, pg, pbt, eps, rows, (_Float16*)out); break;
        case 2: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_add_ln<2, false>), grid, block, 0, st, ps, ps, pg, pbt, eps, rows, (_Float16*)out); break;
        case 3: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_add_ln<3, false>), grid, block, 0, st, ps, ps, pg, pbt, eps, rows, (_Float16*)out); break;
        default: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_add_ln<4, false>), grid, block, 0, st, ps, ps, pg, pbt, eps, rows, (_Float16*)out); break;
    }
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

// ---- E14: the projections of a batch (enc_gemm.hpp) ---------------------------------------------------------------------------
template <int BM, int BN>
static void launch_enc_gemm(EncGemm& a, int epi, hipStream_t st) {
    a.tiles_m = (int)((a.T + BM - 1) / BM);
    a.tiles_n = (a.N + BN - 1) / BN;
    const dim3 grid((unsigned)a.tiles_m * (unsigned)a.tiles_n), block(256);
    const size_t lds = (size_t)2 * (BM + BN) * 128;   // <= 64 KiB
    if (epi == ENC_EPI_BIAS) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_gemm<BM, BN, ENC_EPI_BIAS>), grid, block, lds, st, a);
    else if (epi == ENC_EPI_GELU) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_gemm<BM, BN, ENC_EPI_GELU>), grid, block, lds, st, a);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_enc_gemm<BM, BN, ENC_EPI_RESIDUAL>), grid, block, lds, st, a);
}

extern "C" int rdx_enc_gemm_f16(int device, const void* x, const void* w, const void* bias, const void* res, int64_t n_tokens, int n_out,
                                int n_in, int epilogue, void* out, void* stream) {
    if (n_tokens < 0) return fail(RDX_ERR_INVALID, "rdx_enc_gemm_f16: n_tokens must be >= 0");
    if (n_out < 64 || n_out % 64 || n_in < 64 || n_in % 64) return fail(RDX_ERR_INVALID, "rdx_enc_gemm_f16: n_out and n_in must be multiples of 64");
    if (epilogue < 0 || epilogue > 2) return fail(RDX_ERR_INVALID, "rdx_enc_gemm_f16: epilogue is 0 (bias), 1 (bias + erf GELU) or 2 (bias + residual)");
    if (epilogue == ENC_EPI_RESIDUAL && !res) return fail(RDX_ERR_INVALID, "rdx_enc_gemm_f16: epilogue 2 needs the residual");
    {   // the tile count of the shape the launcher will choose: one workgroup of 256 threads each, fewer than 2^32 threads per launch
        const int64_t bm = n_tokens <= ((int64_t)1 << 40) && enc_gemm_large(n_tokens, n_out, n_in) ? 128 : 64;
        if (n_tokens > ((int64_t)1 << 40) || (n_tokens + bm - 1) / bm * ((n_out + bm - 1) / bm) > ENC_MAX_WORKGROUPS)
            return fail(RDX_ERR_INVALID, "rdx_enc_gemm_f16: n_tokens x n_out needs more than 2^24 - 1 tiles");
    }
    if (n_tokens == 0) return RDX_OK;
    if (!x || !w || !bias || !out) return fail(RDX_ERR_INVALID, "rdx_enc_gemm_f16: null pointer");
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)res | (uintptr_t)out) & 15)
        return fail(RDX_ERR_INVALID, "rdx_enc_gemm_f16: pointers must be 16-byte aligned");
    RDX_TRY(check_device_index("rdx_enc_gemm_f16", device));
    HIP_TRY(hipSetDevice(device));
    EncGemm a;
    a.x = (const _Float16*)x;
    a.w = (const _Float16*)w;
    a.bias = (const _Float16*)bias;
    a.res = (const _Float16*)res;
    a.out = (_Float16*)out;
    a.T = n_tokens;
    a.N = n_out;
    a.K = n_in;
    if (enc_gemm_large(n_tokens, n_out, n_in)) launch_enc_gemm<128, 128>(a, epilogue, (hipStream_t)stream);
    else launch_enc_gemm<64, 64>(a, epilogue, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

// ---- the single-question forward: E4..E7 (enc_small.hpp) ----------------------------------------------------------------------
template <int NTB, int KCS, int NPH, int FPB, bool LNPRO, int EPI>
static int launch_enc_stage(int device, const EncStage& a, hipStream_t st) {
    const size_t lds = (size_t)NTB * 16384 + (size_t)NTB * 16 * KCS * 512 * 2;
    auto* fn = k_enc_stage<NTB, KCS, NPH, FPB, LNPRO, EPI>;
    RDX_TRY(dynamic_lds(device, (const void*)fn, lds));
    hipLaunchKernelGGL(fn, dim3((unsigned)(a.N / FPB)), dim3(1024), lds, st, a);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

template <int NTB, int KCS, int NPH>
static int dispatch_enc_stage(int device, const EncStage& a, bool lnpro, int epi, int fpb, hipStream_t st) {
    if (lnpro) {
        if constexpr (NPH == 1) {
            if (epi == ENC_EPI_BIAS) return launch_enc_stage<NTB, KCS, 1, 16, true, ENC_EPI_BIAS>(device, a, st);
            if (epi == ENC_EPI_GELU) return launch_enc_stage<NTB, KCS, 1, 16, true, ENC_EPI_GELU>(device, a, st);
        }
        return fail(RDX_ERR_INVALID, "rdx_enc_stage_f16: the LayerNorm prologue takes n_in 512 or 1024 and epilogue 0 or 1");
    }
#define RDX_ENC_PLAIN(F)                                                                                                   \
    if (fpb == F) {                                                                                                        \
        if (epi == ENC_EPI_BIAS) return launch_enc_stage<NTB, KCS, NPH, F, false, ENC_EPI_BIAS>(device, a, st);            \
        if (epi == ENC_EPI_GELU) return launch_enc_stage<NTB, KCS, NPH, F, false, ENC_EPI_GELU>(device, a, st);            \
        return launch_enc_stage<NTB, KCS, NPH, F, false, ENC_EPI_RESIDUAL>(device, a, st);                                  \
    }
    RDX_ENC_PLAIN(16)
    RDX_ENC_PLAIN(8)
    RDX_ENC_PLAIN(4)
#undef RDX_ENC_PLAIN
    return fail(RDX_ERR_INVALID, "rdx_enc_stage_f16: features_per_workgroup is 16, 8 or 4");
}

extern "C" int rdx_enc_stage_f16(int device, const void* x, const int64_t* x_rows, const void* ln_gamma, const void* ln_beta, float ln_eps,
                                 void* y_out, const void* w, const void* bias, const void* res, int n_tokens, int n_out, int n_in,
                                 int epilogue, int features_per_workgroup, void* out, void* stream) {
    if (n_tokens < 0 || n_tokens > 32) return fail(RDX_ERR_INVALID, "rdx_enc_stage_f16: at most 32 tokens");
    if (n_in != 512 && n_in != 1024 && n_in != 2048 && n_in != 4096) return fail(RDX_ERR_INVALID, "rdx_enc_stage_f16: n_in must be 512, 1024, 2048 or 4096");
    if (epilogue < 0 || epilogue > 2) return fail(RDX_ERR_INVALID, "rdx_enc_stage_f16: epilogue is 0 (bias), 1 (bias + erf GELU) or 2 (bias + residual)");
    int fpb = features_per_workgroup ? features_per_workgroup : 16;
    if (n_out < fpb || n_out % fpb) return fail(RDX_ERR_INVALID, "rdx_enc_stage_f16: n_out must be a multiple of features_per_workgroup");
    const bool lnpro = ln_gamma != nullptr;
    if (lnpro && (!ln_beta || x_rows)) return fail(RDX_ERR_INVALID, "rdx_enc_stage_f16: the LayerNorm prologue needs gamma and beta and takes no row list");
    if (lnpro && fpb != 16) return fail(RDX_ERR_INVALID, "rdx_enc_stage_f16: the LayerNorm prologue runs with 16 features per workgroup");
    if (epilogue == 2 && !res) return fail(RDX_ERR_INVALID, "rdx_enc_stage_f16: epilogue 2 needs the residual");
    if (n_tokens == 0) return RDX_OK;
    if (!x || !w || !bias || !out) return fail(RDX_ERR_INVALID, "rdx_enc_stage_f16: null pointer");
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)out | (uintptr_t)y_out | (uintptr_t)ln_gamma | (uintptr_t)ln_beta) & 15)
        return fail(RDX_ERR_INVALID, "rdx_enc_stage_f16: pointers must be 16-byte aligned");
    RDX_TRY(check_device_index("rdx_enc_stage_f16", device));
    HIP_TRY(hipSetDevice(device));
    EncStage a;
    a.x = (const _Float16*)x;
    a.x_rows = x_rows;
    a.gamma = (const _Float16*)ln_gamma;
    a.beta = (const _Float16*)ln_beta;
    a.eps = ln_eps;
    a.y_out = (_Float16*)y_out;
    a.w = (const _Float16*)w;
    a.bias = (const _Float16*)bias;
    a.res = (const _Float16*)res;
    a.out = (_Float16*)out;
    a.T = n_tokens;
    a.N = n_out;
    hipStream_t st = (hipStream_t)stream;
#define RDX_ENC_K(NTB)                                                                         \
    switch (n_in) {                                                                            \
        case 512: return dispatch_enc_stage<NTB, 1, 1>(device, a, lnpro, epilogue, fpb, st);   \
        case 1024: return dispatch_enc_stage<NTB, 2, 1>(device, a, lnpro, epilogue, fpb, st);  \
        case 2048: return dispatch_enc_stage<NTB, 2, 2>(device, a, lnpro, epilogue, fpb, st);  \
        default: return dispatch_enc_stage<NTB, 2, 4>(device, a, lnpro, epilogue, fpb, st);    \
    }
    if (n_tokens <= 16) { RDX_ENC_K(1) }
    RDX_ENC_K(2)
#undef RDX_ENC_K
}

extern "C" int rdx_enc_attention_small_f16(int device, const void* qkv, const int32_t* tok_first, int n_tokens, int heads, int head_dim,
                                           float scale, void* ctx, void* stream) {
    if (n_tokens < 0 || n_tokens > 32) return fail(RDX_ERR_INVALID, "rdx_enc_attention_small_f16: at most 32 tokens");
    if (heads < 1 || heads > 65535 || head_dim != ENC_HEAD_DIM) return fail(RDX_ERR_INVALID, "rdx_enc_attention_small_f16: head_dim must be 64");
    if (n_tokens == 0) return RDX_OK;
    if (!qkv || !tok_first || !ctx) return fail(RDX_ERR_INVALID, "rdx_enc_attention_small_f16: null pointer");
    if (((uintptr_t)qkv | (uintptr_t)ctx) & 15) return fail(RDX_ERR_INVALID, "rdx_enc_attention_small_f16: qkv and ctx must be 16-byte aligned");
    RDX_TRY(check_device_index("rdx_enc_attention_small_f16", device));
    HIP_TRY(hipSetDevice(device));
    const float sl2 = scale * 1.4426950408889634f;
    if (n_tokens <= 16)
        hipLaunchKernelGGL(k_enc_attn_small<1>, dim3((unsigned)heads), dim3(64), 0, (hipStream_t)stream, (const _Float16*)qkv, tok_first, n_tokens, heads, sl2, (_Float16*)ctx);
    else
        hipLaunchKernelGGL(k_enc_attn_small<2>, dim3((unsigned)heads), dim3(128), 0, (hipStream_t)stream, (const _Float16*)qkv, tok_first, n_tokens, heads, sl2, (_Float16*)ctx);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_enc_embed_f16(int device, const int64_t* tok, const int64_t* pos_id, const void* word, const void* pos, const void* type0,
                                 int n_tokens, int hidden, void* out, void* stream) {
    if (n_tokens < 0 || hidden < 512 || hidden > 2048 || hidden % 512) return fail(RDX_ERR_INVALID, "rdx_enc_embed_f16: hidden must be 512, 1024, 1536 or 2048");
    if (n_tokens == 0) return RDX_OK;
    if (!tok || !pos_id || !word || !pos || !type0 || !out) return fail(RDX_ERR_INVALID, "rdx_enc_embed_f16: null pointer");
    if (((uintptr_t)word | (uintptr_t)pos | (uintptr_t)type0 | (uintptr_t)out) & 15) return fail(RDX_ERR_INVALID, "rdx_enc_embed_f16: pointers must be 16-byte aligned");
    RDX_TRY(check_device_index("rdx_enc_embed_f16", device));
    HIP_TRY(hipSetDevice(device));
    const dim3 grid((unsigned)((n_tokens + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const _Float16 *pw = (const _Float16*)word, *pp = (const _Float16*)pos, *pt = (const _Float16*)type0;
    switch (hidden / 512) {
        case 1: hipLaunchKernelGGL(k_enc_embed<1>, grid, block, 0, st, tok, pos_id, pw, pp, pt, n_tokens, (_Float16*)out); break;
        case 2: hipLaunchKernelGGL(k_enc_embed<2>, grid, block, 0, st, tok, pos_id, pw, pp, pt, n_tokens, (_Float16*)out); break;
        case 3: hipLaunchKernelGGL(k_enc_embed<3>, grid, block, 0, st, tok, pos_id, pw, pp, pt, n_tokens, (_Float16*)out); break;
        default: hipLaunchKernelGGL(k_enc_embed<4>, grid, block, 0, st, tok, pos_id, pw, pp, pt, n_tokens, (_Float16*)out); break;
    }
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_enc_layernorm_rows_f16(int device, const void* s, const void* gamma, const void* beta, float eps, int rows, int hidden,
                                          float* out, void* stream) {
    if (rows < 0 || hidden < 512 || hidden > 2048 || hidden % 512) return fail(RDX_ERR_INVALID, "rdx_enc_layernorm_rows_f16: hidden must be 512, 1024, 1536 or 2048");
    if (rows == 0) return RDX_OK;
    if (!s || !gamma || !beta || !out) return fail(RDX_ERR_INVALID, "rdx_enc_layernorm_rows_f16: null pointer");
    if (((uintptr_t)s | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15) return fail(RDX_ERR_INVALID, "rdx_enc_layernorm_rows_f16: pointers must be 16-byte aligned");
    RDX_TRY(check_device_index("rdx_enc_layernorm_rows_f16", device));
    HIP_TRY(hipSetDevice(device));
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const _Float16 *ps = (const _Float16*)s, *pg = (const _Float16*)gamma, *pb = (const _Float16*)beta;
    switch (hidden / 512) {
        case 1: hipLaunchKernelGGL(k_enc_ln_rows<1>, grid, block, 0, st, ps, pg, pb, eps, rows, out); break;
        case 2: hipLaunchKernelGGL(k_enc_ln_rows<2>, grid, block, 0, st, ps, pg, pb, eps, rows, out); break;
        case 3: hipLaunchKernelGGL(k_enc_ln_rows<3>, grid, block, 0, st, ps, pg, pb, eps, rows, out); break;
        default: hipLaunchKernelGGL(k_enc_ln_rows<4>, grid, block, 0, st, ps, pg, pb, eps, rows, out); break;
    }
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_enc_gelu_f16(int device, void* x, int64_t n, void* stream) {
    if (n < 0 || n % 8) return fail(RDX_ERR_INVALID, "rdx_enc_gelu_f16: n must be a non-negative multiple of 8");
    if (n == 0) return RDX_OK;
    if (!x || ((uintptr_t)x & 15)) return fail(RDX_ERR_INVALID, "rdx_enc_gelu_f16: x must be a 16-byte aligned device pointer");
    RDX_TRY(check_device_index("rdx_enc_gelu_f16", device));
    HIP_TRY(hipSetDevice(device));
    const int64_t n8 = n / 8;
    const unsigned grid = (unsigned)std::min<int64_t>((n8 + 255) / 256, 2048);
    hipLaunchKernelGGL(k_enc_gelu, dim3(grid), dim3(256), 0, (hipStream_t)stream, (_Float16*)x, n8);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

// ------------------------------------------------------------------------------------------------
// cross-encoder reranker: classification head and selection (rerank_kernel.hpp)
// ------------------------------------------------------------------------------------------------
// the head's two kernels over n rows, for both entry points (fn: the entry point's name, range: its bound on n, as its messages say it)
static int launch_rerank_head(const char* fn, int64_t max_n, const char* range, int device, const float* cls, int64_t n, int hidden,
                              const void* w_dense, const void* b_dense, const void* w_out, const void* b_out, double* workspace,
                              float* scores, void* stream) {
    const std::string f(fn);
    if (n < 1 || n > max_n) return fail(RDX_ERR_INVALID, f + ": n must be in " + range);
    if (hidden < 64 || hidden > RERANK_MAX_HIDDEN || hidden % 64) return fail(RDX_ERR_INVALID, f + ": hidden must be a multiple of 64 in [64, 4096]");
    if (!cls || !w_dense || !b_dense || !w_out || !b_out || !workspace || !scores) return fail(RDX_ERR_INVALID, f + ": null pointer");
    if (((uintptr_t)cls | (uintptr_t)w_dense) & 15) return fail(RDX_ERR_INVALID, f + ": cls and w_dense must be 16-byte aligned");
    if (((uintptr_t)b_dense | (uintptr_t)w_out | (uintptr_t)b_out) & 1 || ((uintptr_t)workspace & 7) || ((uintptr_t)scores & 3))
        return fail(RDX_ERR_INVALID, f + ": misaligned pointer");
    RDX_TRY(check_device_index(fn, device));
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    // workgroup (b, y) takes rows [64 y, 64 y + 64) whatever n is, and row r's partials lie at part[b * n + r] (size_t: 2^29 words at
    // the limits), so a row's arithmetic is that of any shorter call
    const int rows = (int)n;
    const int blocks = hidden / RERANK_FEATURES;
    const dim3 grid((unsigned)blocks, (unsigned)((rows + RERANK_ROWS_PER_BLOCK - 1) / RERANK_ROWS_PER_BLOCK));   // y <= 2^14
    const size_t lds = (size_t)RERANK_FEATURES * hidden * sizeof(_Float16);   // <= 64 KiB at hidden 4096
    RDX_TRY(dynamic_lds(device, (const void*)k_rerank_head, lds));
    hipLaunchKernelGGL(k_rerank_head, grid, dim3(RERANK_HEAD_THREADS), lds, st, cls, rows, hidden, (const _Float16*)w_dense,
                       (const _Float16*)b_dense, (const _Float16*)w_out, workspace);
    HIP_TRY(hipGetLastError());
    const int rows_per_block = RERANK_THREADS / 64;                           // K_R2: one wave per row
    hipLaunchKernelGGL(k_rerank_combine, dim3((unsigned)((rows + rows_per_block - 1) / rows_per_block)), dim3(RERANK_THREADS), 0, st,
                       (const double*)workspace, rows, blocks, (const _Float16*)b_out, scores);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_rerank_head_f16(int device, const float* cls, int n, int hidden, const void* w_dense, const void* b_dense,
                                   const void* w_out, const void* b_out, double* workspace, float* scores, void* stream) {
    return launch_rerank_head("rdx_rerank_head_f16", RERANK_MAX_N, "[1, 1024]", device, cls, n, hidden, w_dense, b_dense, w_out, b_out,
                              workspace, scores, stream);
}

// what rdx_rerank_select and rdx_rerank_select_batch check alike (boosted: the batch's, NULL for the single call)
static int check_select_args(const char* fn, const float* scores, const double* boosts, int top_k, int keep_min, const int32_t* order,
                             const double* final_score, const int32_t* count, const int32_t* boosted, int device) {
    const std::string f(fn);
    if (top_k < 0) return fail(RDX_ERR_INVALID, f + ": top_k must be >= 0");
    if (keep_min < 0) return fail(RDX_ERR_INVALID, f + ": keep_min must be >= 0");
    if (!scores || !order || !final_score || !count) return fail(RDX_ERR_INVALID, f + ": null pointer");
    if (((uintptr_t)scores & 3) || ((uintptr_t)boosts & 7) || ((uintptr_t)order & 3) || ((uintptr_t)final_score & 7) || ((uintptr_t)count & 3) ||
        ((uintptr_t)boosted & 3))
        return fail(RDX_ERR_INVALID, f + ": misaligned pointer");
    RDX_TRY(check_device_index(fn, device));
    return RDX_OK;
}

extern "C" int rdx_rerank_select(int device, const float* scores, const double* boosts, int n, int top_k, double min_score,
                                 int keep_min, int32_t* order, double* final_score, int32_t* count, void* stream) {
    if (n < 1 || n > RERANK_MAX_N) return fail(RDX_ERR_INVALID, "rdx_rerank_select: n must be in [1, 1024]");
    RDX_TRY(check_select_args("rdx_rerank_select", scores, boosts, top_k, keep_min, order, final_score, count, nullptr, device));
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(k_rerank_select, dim3(1), dim3(RERANK_MAX_N), 0, (hipStream_t)stream, scores, boosts, n, top_k, min_score,
                       keep_min, order, final_score, count);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

// ------------------------------------------------------------------------------------------------
// topic boost of a question's candidates (topic_kernel.hpp): the boosts rdx_rerank_select reads
// ------------------------------------------------------------------------------------------------
// the alignment and device checks rdx_topic_boost and rdx_topic_boost_batch end their argument checks with (offsets: the single
// call's int32 pair_offsets or the batch's int64 pair_off, aligned to offsets_bytes)
static int check_topic_pointers(const char* fn, const float* table, const int32_t* topic_slots, const int32_t* tag_slots, const int32_t* pairs,
                                const void* offsets, int offsets_bytes, const double* sims, const double* boosts, const double* best_sim,
                                int device) {
    if ((((uintptr_t)table | (uintptr_t)topic_slots | (uintptr_t)tag_slots | (uintptr_t)pairs) & 3) || ((uintptr_t)offsets & (offsets_bytes - 1)) ||
        (((uintptr_t)sims | (uintptr_t)boosts | (uintptr_t)best_sim) & 7))
        return fail(RDX_ERR_INVALID, std::string(fn) + ": misaligned pointer");
    RDX_TRY(check_device_index(fn, device));
    return RDX_OK;
}

extern "C" int rdx_topic_boost(int device, const float* table, int64_t table_rows, int dim, const int32_t* topic_slots, int n_topics,
                               const int32_t* tag_slots, int n_tags, const int32_t* pair_offsets, const int32_t* pairs, int64_t n_pairs,
                               int n, double threshold, double max_boost, double* sims, double* boosts, double* best_sim, void* stream) {
    if (n < 1 || n > TOPIC_MAX_N) return fail(RDX_ERR_INVALID, "rdx_topic_boost: n must be in [1, 1024]");
    if (dim < 1 || dim > TOPIC_MAX_DIM) return fail(RDX_ERR_INVALID, "rdx_topic_boost: dim must be in [1, 4096]");
    if (n_topics < 0 || n_topics > TOPIC_MAX_TOPICS) return fail(RDX_ERR_INVALID, "rdx_topic_boost: n_topics must be in [0, 32]");
    if (n_tags < 0 || n_tags > TOPIC_MAX_CALL_TAGS) return fail(RDX_ERR_INVALID, "rdx_topic_boost: n_tags must be in [0, 65536]");
    if (n_pairs < 0 || n_pairs > (int64_t)n * TOPIC_MAX_TOPICS * TOPIC_MAX_TAGS)
        return fail(RDX_ERR_INVALID, "rdx_topic_boost: n_pairs must be in [0, n * 32 * 64] (at most 64 tags per candidate)");
    if (table_rows < 0 || table_rows > (int64_t)1 << 31) return fail(RDX_ERR_INVALID, "rdx_topic_boost: table_rows must be in [0, 2^31]");
    const bool dots = n_topics > 0 && n_tags > 0;
    if (!pair_offsets || !boosts || (n_pairs > 0 && !pairs)) return fail(RDX_ERR_INVALID, "rdx_topic_boost: null pointer");
    if (dots && ((table_rows > 0 && !table) || !topic_slots || !tag_slots || !sims))   // (an empty table may be NULL: no slot has an embedding)
        return fail(RDX_ERR_INVALID, "rdx_topic_boost: null pointer (table, slots or sims)");
    RDX_TRY(check_topic_pointers("rdx_topic_boost", table, topic_slots, tag_slots, pairs, pair_offsets, 4, sims, boosts, best_sim, device));
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    if (dots) {
        const int64_t waves = (int64_t)n_topics * n_tags;                  // <= 2^21
        hipLaunchKernelGGL(k_topic_sims, dim3((unsigned)((waves + TOPIC_THREADS / 64 - 1) / (TOPIC_THREADS / 64))), dim3(TOPIC_THREADS), 0, st,
                           table, table_rows, dim, topic_slots, n_topics, tag_slots, n_tags, sims);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_topic_replay, dim3((unsigned)((n + TOPIC_THREADS - 1) / TOPIC_THREADS)), dim3(TOPIC_THREADS), 0, st,
                       (const double*)sims, dots ? n_topics : 0, dots ? n_tags : 0, pair_offsets, pairs, n_pairs, n, threshold, max_boost,
                       boosts, best_sim);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

// ------------------------------------------------------------------------------------------------
// the reranker for a batch of questions (rerank_batch_kernel.hpp)
// ------------------------------------------------------------------------------------------------
extern "C" int rdx_rerank_head_rows_f16(int device, const float* cls, int64_t n, int hidden, const void* w_dense, const void* b_dense,
                                        const void* w_out, const void* b_out, double* workspace, float* scores, void* stream) {
    // rdx_rerank_head_f16's two kernels on a taller grid
    return launch_rerank_head("rdx_rerank_head_rows_f16", RERANK_BATCH_MAX_ROWS, "[1, 2^20]", device, cls, n, hidden, w_dense, b_dense, w_out,
                              b_out, workspace, scores, stream);
}

// cand_off [nq + 1]: starts at 0, never decreases, no segment above 1024, at most 2^20 candidates -> the longest segment
static int check_segments(const char* fn, const int32_t* cand_off, int nq, int* longest) {
    if (cand_off[0] != 0) return fail(RDX_ERR_INVALID, std::string(fn) + ": cand_off must start at 0");
    int top = 0;
    for (int q = 0; q < nq; ++q) {
        const int64_t len = (int64_t)cand_off[q + 1] - cand_off[q];
        if (len < 0) return fail(RDX_ERR_INVALID, std::string(fn) + ": cand_off must not decrease");
        if (len > RERANK_MAX_N) return fail(RDX_ERR_INVALID, std::string(fn) + ": a question has at most 1024 candidates");
        top = std::max(top, (int)len);
    }
    if (cand_off[nq] > RERANK_BATCH_MAX_ROWS) return fail(RDX_ERR_INVALID, std::string(fn) + ": at most 2^20 candidates per call");
    *longest = top;
    return RDX_OK;
}

extern "C" int rdx_topic_boost_batch(int device, const float* table, int64_t table_rows, int dim, int nq, const int32_t* topic_off,
                                     const int32_t* topic_slots, const int32_t* tag_off, const int32_t* tag_slots, const int64_t* sim_off,
                                     const int32_t* cand_off, const int64_t* pair_off, const int32_t* pairs, int64_t n_pairs,
                                     double threshold, double max_boost, double* sims, double* boosts, double* best_sim, void* stream) {
    static const char* fn = "rdx_topic_boost_batch";
    if (nq < 1 || nq > RERANK_BATCH_MAX_QUESTIONS) return fail(RDX_ERR_INVALID, "rdx_topic_boost_batch: nq must be in [1, 65535]");
    if (dim < 1 || dim > TOPIC_MAX_DIM) return fail(RDX_ERR_INVALID, "rdx_topic_boost_batch: dim must be in [1, 4096]");
    if (table_rows < 0 || table_rows > (int64_t)1 << 31) return fail(RDX_ERR_INVALID, "rdx_topic_boost_batch: table_rows must be in [0, 2^31]");
    if (n_pairs < 0) return fail(RDX_ERR_INVALID, "rdx_topic_boost_batch: n_pairs must be >= 0");
    if (!pair_off || !boosts || (n_pairs > 0 && !pairs)) return fail(RDX_ERR_INVALID, "rdx_topic_boost_batch: null pointer");
    RDX_TRY(check_topic_pointers(fn, table, topic_slots, tag_slots, pairs, pair_off, 8, sims, boosts, best_sim, device));
    HIP_TRY(hipSetDevice(device));
    const void *d_topic, *d_tag, *d_sim, *d_cand;
    RDX_TRY(shape_array(fn, "topic_off", topic_off, 4, &d_topic));
    RDX_TRY(shape_array(fn, "tag_off", tag_off, 4, &d_tag));
    RDX_TRY(shape_array(fn, "sim_off", sim_off, 8, &d_sim));
    RDX_TRY(shape_array(fn, "cand_off", cand_off, 4, &d_cand));
    int longest = 0;
    RDX_TRY(check_segments(fn, cand_off, nq, &longest));
    if (topic_off[0] < 0 || tag_off[0] < 0 || sim_off[0] < 0)
        return fail(RDX_ERR_INVALID, "rdx_topic_boost_batch: topic_off, tag_off and sim_off must start at 0 or above");
    int64_t most = 0;                                                     // max_q T_q * U_q
    for (int q = 0; q < nq; ++q) {
        const int64_t T = (int64_t)topic_off[q + 1] - topic_off[q], U = (int64_t)tag_off[q + 1] - tag_off[q];
        if (T < 0 || T > TOPIC_MAX_TOPICS) return fail(RDX_ERR_INVALID, "rdx_topic_boost_batch: a question has 0 to 32 topics (topic_off must not decrease)");
        if (U < 0 || U > TOPIC_MAX_CALL_TAGS) return fail(RDX_ERR_INVALID, "rdx_topic_boost_batch: a question has 0 to 65536 distinct tags (tag_off must not decrease)");
        if (sim_off[q + 1] - sim_off[q] < T * U)
            return fail(RDX_ERR_INVALID, "rdx_topic_boost_batch: sim_off leaves question q less than its T_q * U_q similarities");
        most = std::max(most, T * U);
    }
    if (most > 0 && ((table_rows > 0 && !table) || !topic_slots || !tag_slots || !sims))
        return fail(RDX_ERR_INVALID, "rdx_topic_boost_batch: null pointer (table, slots or sims)");
    if (longest == 0) return RDX_OK;                                      // no candidate anywhere: nothing to write
    hipStream_t st = (hipStream_t)stream;
    if (most > 0) {
        const int64_t per = TOPIC_THREADS / 64;
        hipLaunchKernelGGL(k_topic_sims_batch, dim3((unsigned)((most + per - 1) / per), (unsigned)nq), dim3(TOPIC_THREADS), 0, st, table,
                           table_rows, dim, (const int32_t*)d_topic, topic_slots, (const int32_t*)d_tag, tag_slots, (const int64_t*)d_sim, sims);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_topic_replay_batch, dim3((unsigned)((longest + TOPIC_THREADS - 1) / TOPIC_THREADS), (unsigned)nq), dim3(TOPIC_THREADS), 0,
                       st, (const double*)sims, (const int32_t*)d_topic, (const int32_t*)d_tag, (const int64_t*)d_sim, (const int32_t*)d_cand,
                       pair_off, pairs, n_pairs, threshold, max_boost, boosts, best_sim);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

template <int W>
static void launch_select_batch(int nq, hipStream_t st, const float* scores, const double* boosts, const int32_t* cand_off, int top_k,
                                double min_score, int keep_min, int32_t* order, double* final_score, int32_t* count, int32_t* boosted) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rerank_select_batch<W>), dim3((unsigned)nq), dim3(W), 0, st, scores, boosts, cand_off, top_k, min_score,
                       keep_min, order, final_score, count, boosted);
}

extern "C" int rdx_rerank_select_batch(int device, const float* scores, const double* boosts, int nq, const int32_t* cand_off, int top_k,
                                       double min_score, int keep_min, int32_t* order, double* final_score, int32_t* count,
                                       int32_t* boosted, void* stream) {
    static const char* fn = "rdx_rerank_select_batch";
    if (nq < 1 || nq > RERANK_BATCH_MAX_QUESTIONS) return fail(RDX_ERR_INVALID, "rdx_rerank_select_batch: nq must be in [1, 65535]");
    RDX_TRY(check_select_args(fn, scores, boosts, top_k, keep_min, order, final_score, count, boosted, device));
    HIP_TRY(hipSetDevice(device));
    const void* d_cand;
    RDX_TRY(shape_array(fn, "cand_off", cand_off, 4, &d_cand));
    int longest = 0;
    RDX_TRY(check_segments(fn, cand_off, nq, &longest));
    hipStream_t st = (hipStream_t)stream;
    const int32_t* co = (const int32_t*)d_cand;
    if (longest <= RERANK_BATCH_WIDTHS[0])
        launch_select_batch<RERANK_BATCH_WIDTHS[0]>(nq, st, scores, boosts, co, top_k, min_score, keep_min, order, final_score, count, boosted);
    else if (longest <= RERANK_BATCH_WIDTHS[1])
        launch_select_batch<RERANK_BATCH_WIDTHS[1]>(nq, st, scores, boosts, co, top_k, min_score, keep_min, order, final_score, count, boosted);
    else
        launch_select_batch<RERANK_BATCH_WIDTHS[2]>(nq, st, scores, boosts, co, top_k, min_score, keep_min, order, final_score, count, boosted);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}
