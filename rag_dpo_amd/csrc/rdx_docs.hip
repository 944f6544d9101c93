// rdx_docs.hip — the document store and where_document (rdx_docs_*) of include/rdx.h. What it has in common with the metadata
// store (rdx_meta.hip) is in rdx_store.hpp: StoreBase (device, stream, last-use event, lock), check_program and BitmapStage.
#include "rdx_store.hpp"

#include <vector>

#include "doc_kernel.hpp"

using namespace rdx;

// ------------------------------------------------------------------------------------------------
// document store and where_document (doc_kernel.hpp): the rows' UTF-8 text in HBM, scanned for substrings
// ------------------------------------------------------------------------------------------------
struct rdx_docs : StoreBase {
    int64_t rows = 0;
    int64_t used = 0;                  // arena bytes holding text (current and replaced), in front of the DOC_TAIL zero bytes
    int64_t live = 0;                  // padded bytes of the rows' current text
    DevBuf arena;
    std::vector<int64_t> h_start;      // the row table; the device copy and the unit list follow it in docs_sync
    std::vector<int32_t> h_len;
    std::vector<int2> h_units;         // (row, segment) work list of rows [0, synced_rows)
    int64_t synced_rows = 0;           // rows whose table entries and units are on the device (appends extend them in place)
    bool resync = true;                // replace / compact moved rows: table and units are rebuilt whole
    DevBuf start, len, units;
    // the query of rdx_docs_set_query
    int n_leaves = 0, n_short = 0, n_long = 0, n_ops = 0;
    std::vector<int> pass_ext;         // per pass of k_docs_contains: overlap chunks its longest pattern needs
    DevBuf pat, leaves, prog, leaf_bits, tmp_in, tmp_out;
};

static int64_t doc_pad(int64_t n) { return (n + DOC_ALIGN - 1) & ~(int64_t)(DOC_ALIGN - 1); }

// offsets[0] = 0, non-decreasing (strictly increasing when `strict`: patterns are never empty), rows < 2^31 bytes
static int check_offsets(const char* who, const uint8_t* bytes, const int64_t* off, int64_t n, bool strict) {
    if (!off) return fail(RDX_ERR_INVALID, std::string(who) + ": null offsets");
    if (off[0] != 0) return fail(RDX_ERR_INVALID, std::string(who) + ": offsets[0] must be 0");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t l = off[i + 1] - off[i];
        if (l < (strict ? 1 : 0) || l > INT32_MAX - 64)
            return fail(RDX_ERR_INVALID, std::string(who) + ": offsets must be " + (strict ? "strictly increasing" : "non-decreasing") +
                                             " (entry " + std::to_string(i) + " has length " + std::to_string(l) + ")");
    }
    if (off[n] > 0 && !bytes) return fail(RDX_ERR_INVALID, std::string(who) + ": null bytes");
    return RDX_OK;
}

static int docs_reserve(rdx_docs* h, size_t need) { return grow_keep(h->arena, (size_t)h->used, need, "arena"); }

// writes rows' text at the arena tail (padded), through host staging of at most 64 MiB per copy; dst_start[i] = where row i went
static int docs_write_tail(rdx_docs* h, const uint8_t* bytes, const int64_t* off, int64_t n, std::vector<int64_t>& dst_start) {
    int64_t add = 0;
    for (int64_t i = 0; i < n; ++i) add += doc_pad(off[i + 1] - off[i]);
    RDX_TRY(docs_reserve(h, (size_t)(h->used + add + DOC_TAIL)));
    dst_start.resize((size_t)n);
    const int64_t CHUNK = (int64_t)64 << 20;
    std::vector<uint8_t> stage;
    int64_t i = 0;
    while (i < n) {
        const int64_t first = h->used;
        int64_t j = i, bytes_in = 0;
        while (j < n && (j == i || bytes_in + doc_pad(off[j + 1] - off[j]) <= CHUNK)) bytes_in += doc_pad(off[j + 1] - off[j]), ++j;
        stage.assign((size_t)bytes_in, 0);
        int64_t pos = 0;
        for (int64_t r = i; r < j; ++r) {
            const int64_t l = off[r + 1] - off[r];
            if (l) std::memcpy(stage.data() + pos, bytes + off[r], (size_t)l);
            dst_start[(size_t)r] = first + pos;
            pos += doc_pad(l);
        }
        if (bytes_in) HIP_TRY(hipMemcpy((uint8_t*)h->arena.p + first, stage.data(), (size_t)bytes_in, hipMemcpyHostToDevice));
        h->used += bytes_in;
        i = j;
    }
    HIP_TRY(hipMemset((uint8_t*)h->arena.p + h->used, 0, DOC_TAIL));
    return RDX_OK;
}

// rewrites the arena densely with the rows `keep` (strictly ascending), in that order
static int docs_rewrite(rdx_docs* h, const std::vector<int64_t>& keep) {
    const int64_t n = (int64_t)keep.size();
    std::vector<int64_t> src((size_t)n), dst((size_t)n);
    std::vector<int32_t> len((size_t)n);
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        src[(size_t)i] = h->h_start[(size_t)keep[(size_t)i]];
        len[(size_t)i] = h->h_len[(size_t)keep[(size_t)i]];
        dst[(size_t)i] = total;
        total += doc_pad(len[(size_t)i]);
    }
    DevBuf fresh, d_src, d_dst, d_len;
    RDX_TRY(fresh.ensure((size_t)(total + DOC_TAIL)));
    HIP_TRY(hipMemsetAsync(fresh.p, 0, fresh.bytes, h->own_stream));
    if (n > 0) {
        RDX_TRY(d_src.ensure((size_t)n * 8));
        RDX_TRY(d_dst.ensure((size_t)n * 8));
        RDX_TRY(d_len.ensure((size_t)n * 4));
        HIP_TRY(hipMemcpyAsync(d_src.p, src.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->own_stream));
        HIP_TRY(hipMemcpyAsync(d_dst.p, dst.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->own_stream));
        HIP_TRY(hipMemcpyAsync(d_len.p, len.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->own_stream));
        hipLaunchKernelGGL(k_docs_gather, dim3((unsigned)std::min<int64_t>(n, 4096)), dim3(256), 0, h->own_stream,
                           h->arena.as<uint8_t>(), fresh.as<uint8_t>(), d_src.as<int64_t>(), d_dst.as<int64_t>(), d_len.as<int32_t>(), n);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(h->own_stream));
    std::swap(h->arena.p, fresh.p);
    std::swap(h->arena.bytes, fresh.bytes);
    h->h_start = std::move(dst);
    h->h_len = std::move(len);
    h->rows = n;
    h->used = h->live = total;
    h->resync = true;
    return RDX_OK;
}

// device row table and (row, segment) units follow the host table. After appends only the new rows' entries and units are
// built and uploaded (the device buffers grow in place); after a replace or a compaction everything is rebuilt, O(rows).
static int docs_sync(rdx_docs* h) {
    if (h->synced_rows == h->rows && !h->resync) return RDX_OK;
    if (h->resync) {
        h->h_units.clear();
        h->synced_rows = 0;
    }
    h->resync = true;   // stays set if anything below fails: the next call rebuilds from scratch
    const int64_t r0 = h->synced_rows;
    const size_t u0 = h->h_units.size();
    for (int64_t r = r0; r < h->rows; ++r)
        for (int32_t s = 0; (int64_t)s * DOC_SEG < h->h_len[(size_t)r]; ++s) h->h_units.push_back(make_int2((int)r, s));
    const size_t nu = h->h_units.size();
    RDX_TRY(grow_keep(h->start, (size_t)r0 * 8, (size_t)std::max<int64_t>(h->rows, 1) * 8, "row table"));
    RDX_TRY(grow_keep(h->len, (size_t)r0 * 4, (size_t)std::max<int64_t>(h->rows, 1) * 4, "row table"));
    RDX_TRY(grow_keep(h->units, u0 * sizeof(int2), std::max<size_t>(nu, 1) * sizeof(int2), "unit list"));
    if (h->rows > r0) {
        HIP_TRY(hipMemcpy(h->start.as<int64_t>() + r0, h->h_start.data() + r0, (size_t)(h->rows - r0) * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->len.as<int32_t>() + r0, h->h_len.data() + r0, (size_t)(h->rows - r0) * 4, hipMemcpyHostToDevice));
    }
    if (nu > u0) HIP_TRY(hipMemcpy(h->units.as<int2>() + u0, h->h_units.data() + u0, (nu - u0) * sizeof(int2), hipMemcpyHostToDevice));
    h->synced_rows = h->rows;
    h->resync = false;
    return RDX_OK;
}

extern "C" int rdx_docs_create(int device, rdx_docs** out) {
    if (!out) return fail(RDX_ERR_INVALID, "rdx_docs_create: null out pointer");
    *out = nullptr;
    RDX_TRY(check_device("rdx_docs_create: ", device));
    rdx_docs* h = new rdx_docs();
    int rc = h->open("rdx_docs_create", device);
    if (rc == RDX_OK) rc = h->arena.ensure(DOC_TAIL);
    if (rc == RDX_OK) {
        const hipError_t e = hipMemset(h->arena.p, 0, DOC_TAIL);
        if (e != hipSuccess) rc = fail(RDX_ERR_HIP, std::string("rdx_docs_create: ") + hipGetErrorString(e));
    }
    if (rc != RDX_OK) {
        rdx_docs_destroy(h);
        return rc;
    }
    *out = h;
    return RDX_OK;
}

extern "C" int rdx_docs_destroy(rdx_docs* h) {
    if (!h) return RDX_OK;
    h->close();
    delete h;
    return RDX_OK;
}

extern "C" int rdx_docs_append(rdx_docs* h, const uint8_t* bytes, const int64_t* offsets, int64_t n) {
    if (n < 0) return fail(RDX_ERR_INVALID, "rdx_docs_append: n < 0");
    RDX_TRY(check_offsets("rdx_docs_append", bytes, offsets, n, false));
    if (!h) return fail(RDX_ERR_INVALID, "rdx_docs_append: null store");
    if (h->rows + n > INT32_MAX) return fail(RDX_ERR_INVALID, "rdx_docs_append: more than 2^31 - 1 rows");
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(h->wait());
    std::vector<int64_t> at;
    RDX_TRY(docs_write_tail(h, bytes, offsets, n, at));
    for (int64_t i = 0; i < n; ++i) {
        h->h_start.push_back(at[(size_t)i]);
        h->h_len.push_back((int32_t)(offsets[i + 1] - offsets[i]));
        h->live += doc_pad(offsets[i + 1] - offsets[i]);
    }
    h->rows += n;
    return RDX_OK;
}

extern "C" int rdx_docs_replace(rdx_docs* h, const int64_t* row_ids, const uint8_t* bytes, const int64_t* offsets, int64_t n) {
    if (n < 0 || (n > 0 && !row_ids)) return fail(RDX_ERR_INVALID, "rdx_docs_replace: bad argument");
    RDX_TRY(check_offsets("rdx_docs_replace", bytes, offsets, n, false));
    if (!h) return fail(RDX_ERR_INVALID, "rdx_docs_replace: null store");
    std::lock_guard<std::mutex> lk(h->mu);
    for (int64_t i = 0; i < n; ++i)
        if (row_ids[i] < 0 || row_ids[i] >= h->rows)
            return fail(RDX_ERR_INVALID, "rdx_docs_replace: row id " + std::to_string(row_ids[i]) + " out of range [0, " + std::to_string(h->rows) + ")");
    RDX_TRY(h->wait());
    std::vector<int64_t> at;
    RDX_TRY(docs_write_tail(h, bytes, offsets, n, at));
    for (int64_t i = 0; i < n; ++i) {
        const size_t r = (size_t)row_ids[i];
        h->live += doc_pad(offsets[i + 1] - offsets[i]) - doc_pad(h->h_len[r]);
        h->h_start[r] = at[(size_t)i];
        h->h_len[r] = (int32_t)(offsets[i + 1] - offsets[i]);
    }
    h->resync = true;
    if (h->used - h->live > std::max<int64_t>(h->live, (int64_t)16 << 20)) {   // replaced text outweighs the live text: rewrite
        std::vector<int64_t> all((size_t)h->rows);
        for (int64_t r = 0; r < h->rows; ++r) all[(size_t)r] = r;
        RDX_TRY(docs_rewrite(h, all));
    }
    return RDX_OK;
}

extern "C" int rdx_docs_compact(rdx_docs* h, const int64_t* keep, int64_t n_keep) {
    if (!h || n_keep < 0 || (n_keep > 0 && !keep)) return fail(RDX_ERR_INVALID, "rdx_docs_compact: bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    for (int64_t i = 0; i < n_keep; ++i) {
        if (keep[i] < 0 || keep[i] >= h->rows) return fail(RDX_ERR_INVALID, "rdx_docs_compact: row id out of range");
        if (i > 0 && keep[i] <= keep[i - 1]) return fail(RDX_ERR_INVALID, "rdx_docs_compact: keep list must be strictly ascending");
    }
    RDX_TRY(h->wait());
    return docs_rewrite(h, std::vector<int64_t>(keep, keep + n_keep));
}

extern "C" int rdx_docs_stats(const rdx_docs* h, int64_t* rows, int64_t* live_bytes, int64_t* arena_bytes) {
    if (!h || !rows || !live_bytes || !arena_bytes) return fail(RDX_ERR_INVALID, "rdx_docs_stats: null pointer");
    *rows = h->rows;
    *live_bytes = h->live;
    *arena_bytes = h->used;
    return RDX_OK;
}

extern "C" int rdx_docs_set_query(rdx_docs* h, const uint8_t* pat_bytes, const int64_t* pat_off, int P, const int32_t* program, int n_ops) {
    if (P < 1 || P > RDX_DOCS_MAX_LEAVES)
        return fail(RDX_ERR_INVALID, "rdx_docs_set_query: P must be in [1, " + std::to_string(RDX_DOCS_MAX_LEAVES) + "] (got " + std::to_string(P) + ")");
    if (!pat_bytes) return fail(RDX_ERR_INVALID, "rdx_docs_set_query: null pattern bytes");
    RDX_TRY(check_offsets("rdx_docs_set_query", pat_bytes, pat_off, P, true));
    if (n_ops < 0 || n_ops > FILTER_MAX_OPS || (n_ops > 0 && !program))
        return fail(RDX_ERR_INVALID, "rdx_docs_set_query: need 0 <= n_ops <= " + std::to_string(FILTER_MAX_OPS) + " and a program when n_ops > 0");
    RDX_TRY(check_program("rdx_docs_set_query: ", "P", program, n_ops, P));
    if (!h) return fail(RDX_ERR_INVALID, "rdx_docs_set_query: null store");
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(h->wait());
    std::vector<DocLeaf> shorts, longs;
    for (int p = 0; p < P; ++p) {
        DocLeaf lf;
        lf.off = pat_off[p];
        lf.len = (int32_t)(pat_off[p + 1] - pat_off[p]);
        lf.slot = p;
        const int k = std::min(lf.len, 4);
        lf.prefix = 0;
        for (int b = 0; b < k; ++b) lf.prefix |= (uint32_t)pat_bytes[lf.off + b] << (8 * b);
        lf.pmask = k == 4 ? 0xffffffffu : ((1u << (8 * k)) - 1u);
        (lf.len <= DOC_STAGE_MAX ? shorts : longs).push_back(lf);
    }
    h->pass_ext.clear();
    for (size_t a = 0; a < shorts.size(); a += DOC_LEAVES_PER_PASS) {
        int max_len = 1;
        for (size_t b = a; b < std::min(shorts.size(), a + DOC_LEAVES_PER_PASS); ++b) max_len = std::max(max_len, shorts[b].len);
        h->pass_ext.push_back(std::max(1, (DOC_SEG - 2 + max_len) / 16 - (DOC_SEG / 16 - 1)));   // chunks up to byte 1022 + max_len
    }
    std::vector<DocLeaf> all(shorts);
    all.insert(all.end(), longs.begin(), longs.end());
    RDX_TRY(h->pat.ensure((size_t)pat_off[P]));
    RDX_TRY(h->leaves.ensure(all.size() * sizeof(DocLeaf)));
    RDX_TRY(h->prog.ensure((size_t)std::max(n_ops, 1) * 4));
    HIP_TRY(hipMemcpy(h->pat.p, pat_bytes, (size_t)pat_off[P], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->leaves.p, all.data(), all.size() * sizeof(DocLeaf), hipMemcpyHostToDevice));
    if (n_ops) HIP_TRY(hipMemcpy(h->prog.p, program, (size_t)n_ops * 4, hipMemcpyHostToDevice));
    h->n_leaves = P;
    h->n_short = (int)shorts.size();
    h->n_long = (int)longs.size();
    h->n_ops = n_ops;
    return RDX_OK;
}

// the leaf bitmaps [P][words] of the current query into h->leaf_bits, enqueued on st (the caller holds h->mu and has waited)
static int docs_run_leaves(rdx_docs* h, hipStream_t st) {
    if (h->n_leaves == 0) return fail(RDX_ERR_STATE, "rdx_docs: no query set (rdx_docs_set_query)");
    RDX_TRY(docs_sync(h));
    const int64_t words = (h->rows + 31) / 32;
    const size_t lb = (size_t)h->n_leaves * (size_t)std::max<int64_t>(words, 1) * 4;
    RDX_TRY(h->leaf_bits.ensure(lb));
    HIP_TRY(hipMemsetAsync(h->leaf_bits.p, 0, lb, st));
    if ((int64_t)h->h_units.size() == 0) return RDX_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(((int64_t)h->h_units.size() + DOC_WAVES - 1) / DOC_WAVES, 2048);
    const DocLeaf* lv = h->leaves.as<DocLeaf>();
    for (int a = 0, pass = 0; a < h->n_short; a += DOC_LEAVES_PER_PASS, ++pass) {
        hipLaunchKernelGGL(k_docs_contains, dim3(grid), dim3(DOC_THREADS), 0, st, h->arena.as<uint8_t>(), h->start.as<int64_t>(),
                           h->len.as<int32_t>(), h->units.as<int2>(), (int64_t)h->h_units.size(), lv + a, std::min(DOC_LEAVES_PER_PASS, h->n_short - a),
                           h->pat.as<uint8_t>(), h->pass_ext[(size_t)pass], h->leaf_bits.as<uint32_t>(), words);
        HIP_TRY(hipGetLastError());
    }
    if (h->n_long) {
        hipLaunchKernelGGL(k_docs_contains_long, dim3(grid), dim3(DOC_THREADS), 0, st, h->arena.as<uint8_t>(), h->start.as<int64_t>(),
                           h->len.as<int32_t>(), h->units.as<int2>(), (int64_t)h->h_units.size(), lv + h->n_short, h->n_long, h->pat.as<uint8_t>(),
                           h->leaf_bits.as<uint32_t>(), words);
        HIP_TRY(hipGetLastError());
    }
    return RDX_OK;
}

extern "C" int rdx_docs_contains(rdx_docs* h, uint32_t* out_bits, int space, void* stream) {
    if (!h || !out_bits) return fail(RDX_ERR_INVALID, "rdx_docs_contains: null pointer");
    RDX_TRY(check_space(space));
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(h->wait());
    hipStream_t st = h->stream_for(space, stream);
    RDX_TRY(docs_run_leaves(h, st));
    const size_t bytes = (size_t)h->n_leaves * (size_t)((h->rows + 31) / 32) * 4;
    if (bytes) HIP_TRY(hipMemcpyAsync(out_bits, h->leaf_bits.p, bytes, space == RDX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    return h->finish(space, st);
}

extern "C" int rdx_docs_filter(rdx_docs* h, const uint32_t* base_bits, uint32_t* out_bits, int space, void* stream) {
    if (!h || !out_bits) return fail(RDX_ERR_INVALID, "rdx_docs_filter: null pointer");
    RDX_TRY(check_space(space));
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->n_ops == 0) return fail(RDX_ERR_STATE, "rdx_docs_filter: the query has no program (rdx_docs_set_query with n_ops > 0)");
    RDX_TRY(h->wait());
    const int64_t words = (h->rows + 31) / 32;   // 0: nothing is copied or launched, the event is still recorded
    BitmapStage g;
    RDX_TRY(g.begin(*h, space, stream, words, base_bits, out_bits, h->tmp_in, h->tmp_out));
    RDX_TRY(docs_run_leaves(h, g.st));
    if (words) {
        hipLaunchKernelGGL(k_docs_eval, dim3((unsigned)((words + DOC_EVAL_THREADS - 1) / DOC_EVAL_THREADS)), dim3(DOC_EVAL_THREADS), 0, g.st,
                           h->leaf_bits.as<uint32_t>(), words, h->rows, h->prog.as<int32_t>(), h->n_ops, g.base, g.out);
        HIP_TRY(hipGetLastError());
    }
    return g.end(*h, space, words, out_bits);
}
