// rdx_meta.hip — the metadata store and the `where` predicate scan (rdx_meta_*) of include/rdx.h. What it has in common with the
// document store (rdx_docs.hip) is in rdx_store.hpp: StoreBase (device, stream, last-use event, lock), check_program and BitmapStage.
#include "rdx_store.hpp"

#include <vector>

#include "meta_kernel.hpp"

using namespace rdx;

static_assert(sizeof(rdx_meta_leaf) == sizeof(MetaLeaf) && sizeof(MetaLeaf) == 24, "the leaf of include/rdx.h and the kernel's must agree");

// ------------------------------------------------------------------------------------------------
// metadata columns in HBM (meta_kernel.hpp states the layout), scanned by k_meta_filter
// ------------------------------------------------------------------------------------------------
struct MetaColumn {
    int64_t rows = 0;
    DevBuf kind, pay;
};

struct rdx_meta : StoreBase {   // last_use is recorded behind every filter kernel
    int max_blocks = 1;
    std::vector<MetaColumn*> cols;     // by slot; null = never used
    // the query of rdx_meta_set_query; n_ops = 0: none set, or unset by a change of the store
    int n_leaves = 0, n_ops = 0;
    bool sorted = false;
    std::vector<int> used;             // the slots the query names = the rows of the device column table
    DevBuf leaves, prog, coltab, tmp_in, tmp_out;
};

static constexpr int64_t META_STAGE_ROWS = (int64_t)1 << 22;   // rows per staged upload (32 MiB of payload)

static int meta_check_col(const char* who, int col) {
    if (col < 0 || col >= RDX_META_MAX_COLUMNS)
        return fail(RDX_ERR_INVALID, std::string(who) + ": column slot " + std::to_string(col) + " out of range [0, " + std::to_string(RDX_META_MAX_COLUMNS) + ")");
    return RDX_OK;
}

extern "C" int rdx_meta_create(int device, rdx_meta** out) {
    if (!out) return fail(RDX_ERR_INVALID, "rdx_meta_create: null out pointer");
    *out = nullptr;
    RDX_TRY(check_device("rdx_meta_create: ", device));
    rdx_meta* h = new rdx_meta();
    int cus = 0;
    int rc = h->open("rdx_meta_create", device);
    if (rc == RDX_OK) {
        const hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        if (e != hipSuccess) rc = fail(RDX_ERR_HIP, std::string("rdx_meta_create: ") + hipGetErrorString(e));
    }
    if (rc != RDX_OK) {
        rdx_meta_destroy(h);
        return rc;
    }
    h->max_blocks = std::max(cus, 1) * (2048 / META_THREADS);   // every wave slot of the device once; more rows go grid-stride
    *out = h;
    return RDX_OK;
}

extern "C" int rdx_meta_destroy(rdx_meta* h) {
    if (!h) return RDX_OK;
    h->close();
    for (MetaColumn* c : h->cols) delete c;
    delete h;
    return RDX_OK;
}

extern "C" int rdx_meta_set_rows(rdx_meta* h, int col, int64_t first_row, const uint8_t* kind, const double* num, const int32_t* code, int64_t n) {
    RDX_TRY(meta_check_col("rdx_meta_set_rows", col));
    if (first_row < 0 || n < 0 || first_row + n > INT32_MAX) return fail(RDX_ERR_INVALID, "rdx_meta_set_rows: need first_row >= 0, n >= 0 and at most 2^31 - 1 rows");
    if (n > 0 && (!kind || !num || !code)) return fail(RDX_ERR_INVALID, "rdx_meta_set_rows: null kind / num / code");
    for (int64_t i = 0; i < n; ++i)
        if (kind[i] > 4) return fail(RDX_ERR_INVALID, "rdx_meta_set_rows: kind[" + std::to_string(i) + "] = " + std::to_string(kind[i]) + " is not one of 0 .. 4");
    if (!h) return fail(RDX_ERR_INVALID, "rdx_meta_set_rows: null store");
    std::lock_guard<std::mutex> lk(h->mu);
    h->n_ops = 0;
    if (n == 0) return RDX_OK;
    RDX_TRY(h->wait());
    if ((size_t)col >= h->cols.size()) h->cols.resize((size_t)col + 1, nullptr);
    if (!h->cols[(size_t)col]) h->cols[(size_t)col] = new MetaColumn();
    MetaColumn* c = h->cols[(size_t)col];
    const int64_t end = std::max(c->rows, first_row + n);
    RDX_TRY(grow_keep(c->kind, (size_t)c->rows, (size_t)end, "metadata column"));
    RDX_TRY(grow_keep(c->pay, (size_t)c->rows * 8, (size_t)end * 8, "metadata column"));
    if (first_row > c->rows) {   // the gap is "missing"
        HIP_TRY(hipMemset(c->kind.as<uint8_t>() + c->rows, 0, (size_t)(first_row - c->rows)));
        HIP_TRY(hipMemset(c->pay.as<double>() + c->rows, 0, (size_t)(first_row - c->rows) * 8));
    }
    std::vector<double> stage;
    for (int64_t a = 0; a < n; a += META_STAGE_ROWS) {
        const int64_t m = std::min(META_STAGE_ROWS, n - a);
        stage.resize((size_t)m);
        for (int64_t i = 0; i < m; ++i) {
            const uint8_t kd = kind[a + i];
            stage[(size_t)i] = kd == 0 ? 0.0 : (kd == 1 ? (double)code[a + i] : num[a + i]);
        }
        HIP_TRY(hipMemcpy(c->kind.as<uint8_t>() + first_row + a, kind + a, (size_t)m, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->pay.as<double>() + first_row + a, stage.data(), (size_t)m * 8, hipMemcpyHostToDevice));
    }
    c->rows = end;
    return RDX_OK;
}

extern "C" int rdx_meta_drop_column(rdx_meta* h, int col) {
    RDX_TRY(meta_check_col("rdx_meta_drop_column", col));
    if (!h) return fail(RDX_ERR_INVALID, "rdx_meta_drop_column: null store");
    std::lock_guard<std::mutex> lk(h->mu);
    h->n_ops = 0;
    if ((size_t)col >= h->cols.size() || !h->cols[(size_t)col]) return RDX_OK;
    RDX_TRY(h->wait());
    delete h->cols[(size_t)col];
    h->cols[(size_t)col] = nullptr;
    return RDX_OK;
}

extern "C" int rdx_meta_truncate(rdx_meta* h, int64_t rows) {
    if (rows < 0) return fail(RDX_ERR_INVALID, "rdx_meta_truncate: rows < 0");
    if (!h) return fail(RDX_ERR_INVALID, "rdx_meta_truncate: null store");
    std::lock_guard<std::mutex> lk(h->mu);
    h->n_ops = 0;
    for (MetaColumn* c : h->cols)
        if (c) c->rows = std::min(c->rows, rows);
    return RDX_OK;
}

extern "C" int rdx_meta_stats(const rdx_meta* h, int64_t* columns, int64_t* bytes) {
    if (!h || !columns || !bytes) return fail(RDX_ERR_INVALID, "rdx_meta_stats: null pointer");
    *columns = *bytes = 0;
    for (const MetaColumn* c : h->cols) {
        if (!c) continue;
        *columns += c->rows > 0;
        *bytes += (int64_t)(c->kind.bytes + c->pay.bytes);
    }
    return RDX_OK;
}

extern "C" int rdx_meta_set_query(rdx_meta* h, const rdx_meta_leaf* leaves, int n_leaves, const int32_t* program, int n_ops) {
    const std::string who = "rdx_meta_set_query: ";
    if (n_leaves < 1 || n_leaves > META_MAX_LEAVES || !leaves)
        return fail(RDX_ERR_INVALID, who + "need 1 <= n_leaves <= " + std::to_string(META_MAX_LEAVES) + " and a leaf table (got " + std::to_string(n_leaves) + ")");
    if (n_ops < 1 || n_ops > FILTER_MAX_OPS || !program)
        return fail(RDX_ERR_INVALID, who + "need 1 <= n_ops <= " + std::to_string(FILTER_MAX_OPS) + " and a program (got " + std::to_string(n_ops) + ")");
    for (int i = 0; i < n_leaves; ++i) {
        const rdx_meta_leaf& lf = leaves[i];
        if (lf.op < RDX_META_EQ || lf.op > RDX_META_CONST1) return fail(RDX_ERR_INVALID, who + "leaf " + std::to_string(i) + " has an unknown op");
        if (lf.op >= RDX_META_CONST0) continue;
        RDX_TRY(meta_check_col("rdx_meta_set_query", lf.col));
        if (lf.kind < 1 || lf.kind > 4) return fail(RDX_ERR_INVALID, who + "leaf " + std::to_string(i) + " has a kind outside 1 .. 4");
        if (lf.kind == 1 && lf.op != RDX_META_EQ) return fail(RDX_ERR_INVALID, who + "leaf " + std::to_string(i) + " orders strings: a str leaf takes EQ only");
    }
    RDX_TRY(check_program(who, "n_leaves", program, n_ops, n_leaves));
    if (!h) return fail(RDX_ERR_INVALID, who + "null store");
    std::lock_guard<std::mutex> lk(h->mu);
    for (int i = 0; i < n_leaves; ++i) {
        const rdx_meta_leaf& lf = leaves[i];
        if (lf.op >= RDX_META_CONST0) continue;
        if ((size_t)lf.col >= h->cols.size() || !h->cols[(size_t)lf.col] || h->cols[(size_t)lf.col]->rows == 0)
            return fail(RDX_ERR_INVALID, who + "leaf " + std::to_string(i) + " names column slot " + std::to_string(lf.col) + ", which holds no rows");
    }
    // the kernel's tables: the distinct slots in order of first use; leaves that index them; up to META_SORTED_LEAVES leaves are
    // ordered by column (stable) and the program renumbered, so that the scan loads every column once
    std::vector<int> used, slot_ix(h->cols.size(), -1);
    std::vector<MetaLeaf> lv((size_t)n_leaves);
    for (int i = 0; i < n_leaves; ++i) {
        const rdx_meta_leaf& lf = leaves[i];
        MetaLeaf& o = lv[(size_t)i];
        o.op = lf.op, o.kind = lf.kind, o.code = lf.code;
        o.num = lf.kind == 1 ? (double)lf.code : lf.num;
        o.col = -1;
        if (lf.op >= RDX_META_CONST0) continue;
        if (slot_ix[(size_t)lf.col] < 0) {
            slot_ix[(size_t)lf.col] = (int)used.size();
            used.push_back(lf.col);
        }
        o.col = slot_ix[(size_t)lf.col];
    }
    std::vector<int32_t> prog(program, program + n_ops);
    const bool sorted = n_leaves <= META_SORTED_LEAVES;
    if (sorted) {
        std::vector<int> order((size_t)n_leaves), where_now((size_t)n_leaves);
        for (int i = 0; i < n_leaves; ++i) order[(size_t)i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lv[(size_t)a].col < lv[(size_t)b].col; });
        std::vector<MetaLeaf> by_col((size_t)n_leaves);
        for (int i = 0; i < n_leaves; ++i) by_col[(size_t)i] = lv[(size_t)order[(size_t)i]], where_now[(size_t)order[(size_t)i]] = i;
        lv.swap(by_col);
        for (int32_t& op : prog)
            if (op >= 0) op = where_now[(size_t)op];
    }
    std::vector<MetaCol> tab(std::max<size_t>(used.size(), 1), MetaCol{nullptr, nullptr});
    for (size_t u = 0; u < used.size(); ++u) tab[u] = MetaCol{h->cols[(size_t)used[u]]->kind.as<uint8_t>(), h->cols[(size_t)used[u]]->pay.as<double>()};
    RDX_TRY(h->wait());
    h->n_ops = 0;   // a refused query leaves the one before it in place; one that fails from here on leaves none
    RDX_TRY(h->leaves.ensure(lv.size() * sizeof(MetaLeaf)));
    RDX_TRY(h->prog.ensure(prog.size() * 4));
    RDX_TRY(h->coltab.ensure(tab.size() * sizeof(MetaCol)));
    HIP_TRY(hipMemcpy(h->leaves.p, lv.data(), lv.size() * sizeof(MetaLeaf), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->prog.p, prog.data(), prog.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->coltab.p, tab.data(), tab.size() * sizeof(MetaCol), hipMemcpyHostToDevice));
    h->used = std::move(used);
    h->n_leaves = n_leaves;
    h->sorted = sorted;
    h->n_ops = n_ops;
    return RDX_OK;
}

extern "C" int rdx_meta_filter(rdx_meta* h, int64_t rows, const uint32_t* base_bits, uint32_t* out_bits, int space, void* stream) {
    if (!h || !out_bits) return fail(RDX_ERR_INVALID, "rdx_meta_filter: null pointer");
    RDX_TRY(check_space(space));
    if (rows < 0 || rows > INT32_MAX) return fail(RDX_ERR_INVALID, "rdx_meta_filter: rows must be in [0, 2^31)");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->n_ops == 0) return fail(RDX_ERR_STATE, "rdx_meta_filter: no query set since the store last changed (rdx_meta_set_query)");
    for (int s : h->used)
        if (h->cols[(size_t)s]->rows != rows)
            return fail(RDX_ERR_STATE, "rdx_meta_filter: column slot " + std::to_string(s) + " holds " + std::to_string(h->cols[(size_t)s]->rows) +
                                           " rows, the call says " + std::to_string(rows));
    if (rows == 0) return RDX_OK;
    HIP_TRY(hipSetDevice(h->device));
    const int64_t words = (rows + 31) / 32;
    BitmapStage g;
    RDX_TRY(g.begin(*h, space, stream, words, base_bits, out_bits, h->tmp_in, h->tmp_out));
    const int64_t block_rows = META_THREADS * META_ROWS;
    const unsigned grid = (unsigned)std::min<int64_t>((rows + block_rows - 1) / block_rows, h->max_blocks);
    if (h->sorted)
        hipLaunchKernelGGL(k_meta_filter<true>, dim3(grid), dim3(META_THREADS), 0, g.st, h->coltab.as<MetaCol>(), h->leaves.as<MetaLeaf>(), h->n_leaves,
                           h->prog.as<int32_t>(), h->n_ops, rows, words, g.base, g.out);
    else
        hipLaunchKernelGGL(k_meta_filter<false>, dim3(grid), dim3(META_THREADS), 0, g.st, h->coltab.as<MetaCol>(), h->leaves.as<MetaLeaf>(), h->n_leaves,
                           h->prog.as<int32_t>(), h->n_ops, rows, words, g.base, g.out);
    HIP_TRY(hipGetLastError());
    return g.end(*h, space, words, out_bits);
}
