// rdx_bm25_build.hip — building a BM25 index from text (rdx_bm25_build_*) of include/rdx.h.
#include "rdx_host.hpp"

#include <memory>
#include <mutex>
#include <vector>

#include "bm25_build_kernel.hpp"

using namespace rdx;

// ------------------------------------------------------------------------------------------------
// One build (bm25_build_kernel.hpp): the term table, its counters, and the row tables of every batch tokenised so far. A batch's
// row tables stay until the build is destroyed: its launch may still be running when the next batch arrives.
// ------------------------------------------------------------------------------------------------
struct rdx_bm25_build {
    int device = 0;
    int64_t slots = 0, rows = 0;
    uint64_t hash_mask = 0;
    DevBuf table, counters;
    std::vector<std::unique_ptr<DevBuf>> row_tables;
    hipStream_t last_stream = nullptr;
    std::mutex mu;
};

extern "C" int rdx_bm25_build_create(int device, int64_t table_slots, uint64_t hash_mask, rdx_bm25_build** out) {
    if (!out) return fail(RDX_ERR_INVALID, "rdx_bm25_build_create: null out pointer");
    *out = nullptr;
    if (table_slots < 2 || table_slots > BM25_BUILD_MAX_SLOTS || (table_slots & (table_slots - 1)))
        return fail(RDX_ERR_INVALID, "rdx_bm25_build_create: table_slots must be a power of two in [2, 2^31] (got " +
                                         std::to_string(table_slots) + ")");
    RDX_TRY(check_device("rdx_bm25_build_create: ", device));
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<rdx_bm25_build> h(new rdx_bm25_build());
    h->device = device;
    h->slots = table_slots;
    h->hash_mask = hash_mask;
    RDX_TRY(h->table.ensure((size_t)table_slots * sizeof(Bm25Slot)));
    RDX_TRY(h->counters.ensure(BM25_N_COUNTERS * sizeof(bm25_u64)));
    HIP_TRY(hipMemset(h->counters.p, 0, BM25_N_COUNTERS * sizeof(bm25_u64)));
    const int blocks = (int)std::min<int64_t>((table_slots + 255) / 256, 4096);
    hipLaunchKernelGGL(k_bm25_table_init, dim3(blocks), dim3(256), 0, nullptr, h->table.as<Bm25Slot>(), table_slots);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));   // the table is ready for whichever stream tokenises
    *out = h.release();
    return RDX_OK;
}

extern "C" int rdx_bm25_build_destroy(rdx_bm25_build* h) {
    if (!h) return RDX_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->last_stream);   // a launch may still read the table and the row tables
    delete h;
    return RDX_OK;
}

extern "C" int rdx_bm25_build_tokenize(rdx_bm25_build* h, const uint8_t* text, int64_t text_bytes, const int64_t* row_off,
                                       int64_t n_rows, int64_t row_base, int64_t* keys, int64_t key_cap, int32_t* doc_len,
                                       void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_bm25_build_tokenize: null build");
    if (n_rows < 0 || row_base < 0 || row_base > BM25_BUILD_MAX_ROWS || n_rows > BM25_BUILD_MAX_ROWS - row_base)
        return fail(RDX_ERR_INVALID, "rdx_bm25_build_tokenize: row_base + n_rows must stay below 2^31");
    if (n_rows == 0) return RDX_OK;
    if (!text || !row_off || !doc_len) return fail(RDX_ERR_INVALID, "rdx_bm25_build_tokenize: null pointer");
    if (row_off[0] != 0 || row_off[n_rows] != text_bytes)
        return fail(RDX_ERR_INVALID, "rdx_bm25_build_tokenize: row_off must run from 0 to text_bytes");
    // the rows and the keys' stretches are checked, and the stretches laid out, before anything is enqueued
    std::vector<int64_t> tables(2 * (size_t)n_rows + 2);
    int64_t* key_off = tables.data() + n_rows + 1;
    key_off[0] = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t len = row_off[r + 1] - row_off[r] - 1;   // the row's NUL is not part of it
        if (len < 0 || len > BM25_BUILD_MAX_ROW_BYTES || row_off[r + 1] > text_bytes)
            return fail(RDX_ERR_INVALID, "rdx_bm25_build_tokenize: row " + std::to_string(r) +
                                             ": a row is its bytes and one NUL, at most 2^32 - 1 bytes, inside the text");
        key_off[r + 1] = key_off[r] + (len + 1) / 3;
    }
    if (key_cap < key_off[n_rows] || (key_off[n_rows] > 0 && !keys))
        return fail(RDX_ERR_INVALID, "rdx_bm25_build_tokenize: keys must hold the sum of (len + 1) / 3 over the rows = " +
                                         std::to_string(key_off[n_rows]) + " (got " + std::to_string(key_cap) + ")");
    std::memcpy(tables.data(), row_off, (size_t)(n_rows + 1) * 8);
    std::lock_guard<std::mutex> lock(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    std::unique_ptr<DevBuf> d(new DevBuf());
    RDX_TRY(d->ensure(tables.size() * 8));
    HIP_TRY(hipMemcpy(d->p, tables.data(), tables.size() * 8, hipMemcpyHostToDevice));   // complete on return: the launch may follow
    const int64_t* d_row_off = d->as<int64_t>();
    h->row_tables.push_back(std::move(d));
    h->last_stream = (hipStream_t)stream;
    h->rows += n_rows;
    const int blocks = (int)std::min<int64_t>(n_rows, BM25_TOK_MAX_BLOCKS);
    hipLaunchKernelGGL(k_bm25_tok, dim3(blocks), dim3(BM25_TOK_THREADS), 0, (hipStream_t)stream, text, d_row_off, d_row_off + n_rows + 1,
                       n_rows, row_base, h->table.as<Bm25Slot>(), (bm25_u64)(h->slots - 1), (bm25_u64)h->hash_mask, keys, doc_len,
                       h->counters.as<bm25_u64>());
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_bm25_build_stats(rdx_bm25_build* h, int64_t* terms, int64_t* tokens, int32_t* full) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_bm25_build_stats: null build");
    std::lock_guard<std::mutex> lock(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->last_stream));
    bm25_u64 c[BM25_N_COUNTERS];
    HIP_TRY(hipMemcpy(c, h->counters.p, sizeof(c), hipMemcpyDeviceToHost));
    if (c[BM25_CNT_OVERFLOW])
        return fail(RDX_ERR_STATE, "rdx_bm25_build_stats: a row held more tokens than (len + 1) / 3: the text was not the UTF-8 rows promised");
    if (terms) *terms = (int64_t)c[BM25_CNT_TERMS];
    if (tokens) *tokens = (int64_t)c[BM25_CNT_TOKENS];
    if (full) *full = c[BM25_CNT_FULL] ? 1 : 0;
    return RDX_OK;
}

extern "C" int rdx_bm25_build_first_pos(rdx_bm25_build* h, int64_t* out_first_pos, int64_t n, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_bm25_build_first_pos: null build");
    if (!out_first_pos || n != h->slots)
        return fail(RDX_ERR_INVALID, "rdx_bm25_build_first_pos: out must hold table_slots = " + std::to_string(h->slots) + " entries");
    std::lock_guard<std::mutex> lock(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    if (h->last_stream != (hipStream_t)stream) HIP_TRY(hipStreamSynchronize(h->last_stream));
    HIP_TRY(hipMemcpy2DAsync(out_first_pos, 8, (const char*)h->table.p + offsetof(Bm25Slot, first_pos), sizeof(Bm25Slot), 8, (size_t)n,
                             hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return RDX_OK;
}

extern "C" int rdx_bm25_build_vocab(rdx_bm25_build* h, const int32_t* slots, int64_t n_terms, int64_t* term_off, uint8_t* arena,
                                    int64_t arena_bytes, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_bm25_build_vocab: null build");
    if (n_terms < 0 || n_terms > h->slots || arena_bytes < 0)
        return fail(RDX_ERR_INVALID, "rdx_bm25_build_vocab: n_terms must be in [0, table_slots] and arena_bytes >= 0");
    if (n_terms == 0) return RDX_OK;
    if (!slots || !term_off) return fail(RDX_ERR_INVALID, "rdx_bm25_build_vocab: null pointer");
    std::lock_guard<std::mutex> lock(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    if (h->last_stream != (hipStream_t)stream) HIP_TRY(hipStreamSynchronize(h->last_stream));
    const int blocks = (int)((n_terms + BM25_VOCAB_THREADS - 1) / BM25_VOCAB_THREADS);
    hipLaunchKernelGGL(k_bm25_vocab, dim3(blocks), dim3(BM25_VOCAB_THREADS), 0, (hipStream_t)stream, h->table.as<Bm25Slot>(),
                       (bm25_u64)(h->slots - 1), slots, n_terms, term_off, arena, arena_bytes);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}
