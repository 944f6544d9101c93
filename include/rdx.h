/*
 * rdx.h — C-ABI of librdx, the MI355X (gfx950) dense-retrieval hot path that stands in for
 * RAG-DPO's `embedding_provider.embed(...)` L2-normalise step and Chroma `collection.query(...)`.
 *
 * The reference (MatJoss/RAG-DPO) has no FFI of its own: its boundary is two duck-typed Python
 * objects. Each entry point below names the reference call it replaces; the
 * Python mirror of those objects (rag_dpo_amd/collection.py, embedding_provider.py) binds these
 * symbols with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every function returns 0 (RDX_OK) or an RDX_ERR_* code; rdx_last_error() gives the
 *     thread-local message of the last failure on the calling thread.
 *   - `space` says where EVERY pointer argument of that call lives: RDX_HOST or RDX_DEVICE
 *     (device = the index's HIP device). Caller owns all buffers.
 *   - `stream` is a hipStream_t passed as void*. RDX_DEVICE calls run on exactly that stream (NULL =
 *     HIP's default stream, as with any HIP API), i.e. ordered after whatever the caller enqueued
 *     there to produce the inputs; rdx_search additionally synchronises the stream once before it
 *     returns (overflow check). RDX_HOST calls are synchronous; NULL = the library's own stream.
 *     Calls WITHOUT a stream argument (add / update / get / compact) given RDX_DEVICE pointers first
 *     wait for all work enqueued on the device so far (hipDeviceSynchronize) and are complete on return.
 *   - rows are addressed by their insertion index ("row id", int64, 0-based); the Python layer
 *     maps row ids to Chroma string ids / documents / metadatas.
 *   - scores are cosine similarities in fp32: exact dot product of the two L2-normalised fp32
 *     vectors accumulated in fp64 in a fixed order (oracle/rdx_oracle.c states the order), rounded
 *     once to fp32. Chroma's `distance` is `1.0f - score` ("hnsw:space": "cosine",
 *     reference src/processing/create_chromadb_index.py:100-106).
 *   - result order per query: score descending, ties by ascending row id (= ascending distance,
 *     the order `RAGRetriever._parse_chromadb_results` consumes, reference src/rag/retriever.py:472-494).
 *     Scores are compared as floats: +0 and -0 are the same score for ordering (rows scoring either tie and are ordered by
 *     row id), and the sign of a returned zero is the sign of that row's exact score.
 */
#ifndef RDX_H
#define RDX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDX_OK 0
#define RDX_ERR_INVALID 1 /* bad argument: shape, k, NaN/Inf in input, unknown option */
#define RDX_ERR_HIP 2     /* HIP runtime failure (message carries hipGetErrorString) */
#define RDX_ERR_NOMEM 3   /* device or host allocation failed */
#define RDX_ERR_STATE 4   /* call not valid in the index's current state */

#define RDX_HOST 0
#define RDX_DEVICE 1

#define RDX_ABI_VERSION 3 /* 2: flags word in the packed partial, rdx_signal, rdx_search_async(out_flags); 3: the single-question encoder stages */

typedef struct rdx_index rdx_index; /* opaque: one corpus shard resident in one GPU's HBM */

/* Library / device ---------------------------------------------------------------------------- */
int rdx_version(void);
const char* rdx_last_error(void);
int rdx_device_count(int* n);
/* How the host waits for a search (rdx_search, rdx_search_wait, rdx_signal_wait), process-wide. Default (400, 0): spin on the
 * search's pinned mailbox word for spin_us, then poll it with sched_yield() between looks — lowest latency, one host core busy per
 * waiting thread for the length of the search. sleep_us > 0: after the spin, sleep that long between looks (a server whose
 * sessions share the cores — the reference serves concurrent Streamlit sessions from one process, app.py:42-43 — wants e.g.
 * (50, 100): small searches still end inside the spin, a 15 ms scan costs ~1 % of a core and is noticed <= 100 us late).
 * Environment RDX_WAIT_SPIN_US / RDX_WAIT_SLEEP_US set the initial values. Speed only. */
int rdx_set_wait_policy(int spin_us, int sleep_us);

/* Index lifecycle — replaces chromadb `create_collection(..., {"hnsw:space": "cosine"})` /
 * `get_collection` (reference create_chromadb_index.py:100-106,112; app.py:58-59). */
int rdx_index_create(int device, int dim, rdx_index** out);
int rdx_index_destroy(rdx_index* h);
int rdx_index_dim(const rdx_index* h, int* dim);
/* `collection.count()` (reference src/rag/bm25_index.py:200, app.py:108). */
int rdx_index_count(const rdx_index* h, int64_t* rows);
int rdx_index_reserve(rdx_index* h, int64_t rows);

/* `collection.add(embeddings=...)` (reference create_chromadb_index.py:374-379,
 * ingest_enterprise.py:241-246): append n raw fp32 rows [n][dim]; each is L2-normalised on the
 * device (K1) into the fp32 master copy and the tiled fp16 scan copy. Row ids continue from
 * count(). Rows containing NaN/Inf are rejected (RDX_ERR_INVALID) and nothing is added. */
int rdx_index_add(rdx_index* h, const float* rows, int64_t n, int space);
/* Config 5 (BASELINE.json): corpus delivered as bf16 (raw 16-bit patterns); the master copy
 * holds the bf16 values widened to fp32 and normalised like any other row. */
int rdx_index_add_bf16(rdx_index* h, const uint16_t* rows, int64_t n, int space);
/* Reload of a persisted collection (chromadb's PersistentClient returns stored vectors unchanged, reference app.py:58-59
 * reads what create_chromadb_index.py wrote): rows are values previously returned by rdx_index_get, i.e. already
 * L2-normalised; they are stored VERBATIM (no second normalisation, which could move a component by an ulp), so scores
 * after a reload are bit-identical to those before it. NaN/Inf rows are rejected as in rdx_index_add. */
int rdx_index_add_stored(rdx_index* h, const float* rows, int64_t n, int space);
/* `collection.update(ids=, embeddings=)` / upsert: overwrite existing rows in place. All or nothing: a call with a row id outside
 * [0, count()), a row id given more than once (two rows of one call have no order: RDX_ERR_INVALID, the message names the id) or a
 * row containing NaN/Inf (RDX_ERR_INVALID) is refused before anything is written; every row of the index and every search result
 * is then what it was before the call. */
int rdx_index_update(rdx_index* h, const int64_t* row_ids, const float* rows, int64_t n, int space);
/* rdx_index_update for rows that ARE stored values, as rdx_index_add_stored is to rdx_index_add: written verbatim (the lifted rows
 * of an "ip" / "l2" collection, below). Additive: rdx_index_update is unchanged. Refused under the same rules, as completely: an id
 * out of range or given more than once, or a NaN/Inf row, and nothing is written. */
int rdx_index_update_stored(rdx_index* h, const int64_t* row_ids, const float* rows, int64_t n, int space);
/* `collection.get(include=["embeddings"])`: the stored (normalised) fp32 rows. */
int rdx_index_get(rdx_index* h, const int64_t* row_ids, int64_t n, float* out, int space);
/* `collection.delete(ids=...)` (reference ingest_enterprise.py:272,304): keep exactly the rows
 * listed in `keep` (strictly ascending, host pointer), renumbering them 0..n_keep-1. */
int rdx_index_compact(rdx_index* h, const int64_t* keep, int64_t n_keep);

/* Shards whose rows are not one contiguous range of the collection (several GPUs behind ONE `collection` object, rows
 * dealt to the devices as they arrive): returned row id of local row r = ids[r]. ids must be strictly increasing over the
 * shard (ties inside a shard are ordered by local row, which then is the order of the returned ids too). Sets the ids
 * of rows [first_row, first_row + n), which must exist; rows never given an id return local + "row_base". An index
 * without a map (the default) returns local + "row_base". rdx_index_compact drops the map (rows are renumbered). */
int rdx_index_set_row_ids(rdx_index* h, int64_t first_row, const int64_t* ids, int64_t n, int space);

/* Options (tests and benchmarks): "force_exact" 0/1, "force_fast" 0/1 (MFMA scan even for small
 * problems), "sample_div" >=1, "cand_cap" 0 (auto) or slots per (query, stream) candidate segment,
 * "profile" 0..3: 1 = HIP events around every kernel of the next searches, 2 = two events around the dominant kernel(s) only
 * (main scan, or K5a + K5b on the exact path), 3 = no events: those kernels stamp their own first-workgroup start and
 * last-workgroup end (an event record costs the stream ~6 us, 10 % of a small search) — rdx_search_stats.ms_*; "row_base" >= 0:
 * added to every returned row id, so a shard holding rows [base, base+count) answers with GLOBAL ids;
 * "xcd_balance" 0/1 (default 1): the main scan's
 * tiles are split between the 8 XCDs by their measured speed in the previous searches instead of evenly (the XCDs of
 * one chip differ by up to 10 %; speed only); "compact_master" 0/1 (default 0; only while the index is empty): the exact copy of the rows keeps the raw bf16 rows as
 * delivered by rdx_index_add_bf16 plus one fp64 divisor per row (2 B/element + 8 B/row) instead of the normalised fp32 rows
 * (4 B/element); every normalised element is recomputed as (float)((double)x / den) where the exact re-score, the exact scan
 * and rdx_index_get need it — the operands and the operation of the ingest normalisation, hence the same bits. With the fp16
 * scan copy that is 4 instead of 6 B/element for a bf16 corpus (BASELINE config 5). Such an index takes rows through
 * rdx_index_add_bf16 only (rdx_index_add / _add_stored / _update return RDX_ERR_STATE);
 * "fuse_epilogue" 0/1 (default 1): B > 128 main scan variant whose per-tile emit check rides inside the
 * first k-step of the next tile instead of interrupting the MFMA stream (speed only: +1 % at B = 1024; used when the
 * number of 64-element k-steps per row is even, the stand-alone check otherwise and with 0);
 * "spec_tau" 0/1 (default 1): the scan threshold is taken from a rank below k of the sampled scores — an estimate of the corpus'
 * k-th score instead of a proven lower bound — and verified per query afterwards (c_k - 2E >= threshold); a query that fails
 * takes the fallback passes with the proven threshold (speed only: 2-6x fewer candidates; never results);
 * "split_boot" 0/1 (default 1): searches of <= 64 queries whose threshold sample is small take it with the split-K bootstrap
 * kernel (one 32-row block per workgroup, the k-steps dealt to its waves) instead of whole tiles on a few CUs;
 * "small_scan" 0/1 (default 1): the same searches on corpora of at most 32 such blocks per CU (262 K rows on 256 CUs) take their
 * main scan with the split-K kernel too (balanced in 32-row units instead of whole 256-row tiles);
 * "half_boot" 0/1 (default 1): searches of 129..256 queries take their threshold sample as two 128-query tiles per sampled corpus
 * tile (every CU busy, less data per k-step) instead of one 256-query tile on half the CUs;
 * "spread_boot" 0/1 (default 1): every threshold sample not taken by the split-K bootstrap (see "split_boot"), whatever the batch
 * size, is every div-th 32-row block of the corpus instead of every div-th 256-row tile (the same number of rows, eight times finer:
 * runs of similar rows stored together — a document's chunks — are met by the sample instead of falling between two sampled
 * tiles; such a sample is not thinned to whole rounds of the streams as a tile sample is; speed only);
 * "fuse_finish" 0/1 (default 1): the end-of-search work (counters and small results to pinned host memory) runs in the last
 * block of the search's last kernel instead of a launch of its own (both: speed only);
 * "retry" 0/1 (default 1): queries whose candidate
 * segments overflow get a second MFMA pass as a small batch (denser threshold sample) before the exact full scan;
 * "coarse_i8" 0/1/2 (default 2): the main scan of more than 128 queries at dim_pad <= 1024 (a multiple of 128) on int8 MFMA over a
 * block-scaled int8 copy of the corpus (built by the first search that needs it, +1 B per element; not persisted), with an error
 * bound of its own per query: 0 never, 1 whenever the shape allows, 2 for more than 256 queries on at least 2^20 rows (speed only);
 * "refine_pilot" 0..64 (default 4): an int8 search re-scores its hits in two rounds, the refine_pilot * k best coarse hits first
 * and then the hits within E_q of their exact k-th score; 0 = one band of 2 E_q below the k-th coarse score (speed only);
 * "refine_spill" 0/1/2 (default 2): a query with more scan hits than the refine kernel's list in LDS holds (7 168) is answered from a
 * list in HBM (up to 40 960 hits per query, allocated by the first search that needs it: 320 MB per 1 024 queries) instead of by the
 * fallback passes: 0 never, 1 on every MFMA-path search, 2 where "coarse_i8" = 2 chose the int8 pass (speed only);
 * "i8_sample_mul" 0/1/2/4/8 (default 0): the threshold sample of an int8 search, in multiples of the fp16 pass's (every 64th 32-row
 * block on a large shard): 0 = 2 where "coarse_i8" = 2 chose the int8 pass with "refine_spill" in force, 8 elsewhere (speed only);
 * "i8_eps_classes" 0/1/2/4/8 (default 0): an int8 search's scan charges a 32-row block the quantisation error of its class of blocks
 * (edges at the 50 / 75 / 87.5 ... % quantiles of the blocks' errors, the top class the corpus' largest) instead of the corpus' largest
 * throughout: fewer hits to gather, the same answers; 0 = 8 where "coarse_i8" = 2 chose the int8 pass, 1 elsewhere (speed only);
 * developer options "refine_list" (0 = automatic, or 32..7168: upper bound on the LDS list's entries) and "spill_cap" (0 = automatic,
 * or 32..40960: upper bound on the HBM list's entries) drive the two lists' limits at small sizes (tests);
 * developer option "dup_batch" (0 = automatic, or 1..4096): rows per batch of rdx_index_near_dup (tests: edges across batch borders);
 * developer option "km_tiles" (0 = automatic, or 1..4096): at least this many tiles of 256 rows per block of rdx_index_kmeans' ordering
 * (tests: blocks of several tiles, which the automatic choice takes beyond 2^22 / n_clusters blocks);
 * "facet_table_kb" (0 = the default, 262 144, or 1..4194304): the KiB that the per-query count tables of one pass of
 * rdx_index_range_facets may take (speed and memory only: a pass holds budget / (4 B x n_groups) queries, one at the least). */
int rdx_index_set_option(rdx_index* h, const char* name, int64_t value);

/* The main scan's tile shares of the 8 XCDs (1.0 = an eighth; option "xcd_balance"): learned from the workgroups' own time stamps
 * over the first searches of a process — the first launches of a cold index run with even shares, ~15 % slower on a 10 M-row
 * scan. out8 (may be NULL) receives the current shares; in8 (may be NULL) replaces them (each clamped to [0.6, 1.5], renormalised
 * to sum 8): a host layer that persists an index (rag_dpo_amd/collection.py) stores them with it and hands them back at load.
 * Speed only, never results; they re-adapt if the values no longer fit the device. */
int rdx_index_xcd_shares(rdx_index* h, double* out8, const double* in8);

/* `SentenceTransformer.encode(..., normalize_embeddings=True)`'s last step
 * (reference src/utils/embedding_provider.py:139-145): out[i] = in[i] / max(||in[i]||_2, 1e-12). */
int rdx_l2_normalize(int device, const float* in, int64_t n, int dim, float* out, int space,
                     void* stream);

/* Two fused kernels for the memory-bound parts of the query encoder's forward — what `SentenceTransformer.encode` runs on the
 * GPU in front of that normalisation (reference src/utils/embedding_provider.py:118-147; the projections of a batch are the BLAS library's by default, or
 * rdx_enc_gemm_f16 below: rag_dpo_amd/embedding_provider.py, gemm="blas" | "rdx"). fp16 device pointers, 16-byte aligned; enqueued on `stream`, nothing is synchronised.
 *
 * rdx_enc_attention_f16: self-attention over PACKED tokens (no padding). qkv [n_tokens][3*heads*head_dim]: per token its query,
 *   key and value rows (heads x head_dim each, head-major); token t belongs to the text whose tokens are
 *   tok_first[t] .. tok_first[t] + tok_len[t] - 1 (tok_len >= 1) and attends to exactly those. ctx [n_tokens][heads*head_dim] =
 *   softmax(q k^T * scale) v per head, soft-max and accumulation in fp32. head_dim must be 64. Meant for short texts
 *   (questions): the work per token grows with its text's length. max_text_tokens: the longest text's token count if the caller
 *   knows it (sizes the LDS window a workgroup stages keys in; a wrong or unknown value — pass 0 — costs speed only: rows whose
 *   text does not fit the window read global memory).
 * rdx_enc_add_layernorm_f16: out[r] = LayerNorm(a[r] + b[r]) * gamma + beta over rows of `hidden` halves (512, 1024, 1536 or
 *   2048; biased variance, fp32 statistics, the sum rounded to fp16 first — what an fp16 add followed by LayerNorm computes). */
int rdx_enc_attention_f16(int device, const void* qkv, const int32_t* tok_first, const int32_t* tok_len,
                          int64_t n_tokens, int heads, int head_dim, float scale, int max_text_tokens, void* ctx,
                          void* stream);
/* rdx_enc_attention_mfma_f16: the same attention for texts of ANY length (the corpus side: chunk texts of up to ~1 K tokens, reference
 *   src/processing/create_chromadb_index.py:300-387) on the matrix cores, flash-style. query_blocks [n_blocks][4] int32 =
 *   {first token of the text, its length, first query of this block within the text, 0}: one workgroup per block of <= 64 queries and
 *   head; the caller lists ceil(length / 64) blocks per text. Same arithmetic contract as rdx_enc_attention_f16 (soft-max and
 *   accumulation in fp32; probabilities rounded to fp16 before the PV product, as a flash kernel does). */
int rdx_enc_attention_mfma_f16(int device, const void* qkv, const int32_t* query_blocks, int n_blocks, int heads,
                               int head_dim, float scale, void* ctx, void* stream);
int rdx_enc_add_layernorm_f16(int device, const void* a, const void* b, const void* gamma, const void* beta,
                              float eps, int64_t rows, int hidden, void* out, void* stream);
/* rdx_enc_gelu_f16: x[i] = gelu(x[i]) IN PLACE over n fp16 values (n a multiple of 8, x 16-byte aligned): the erf form the
 *   checkpoint's FFN uses (HF XLMRobertaIntermediate, hidden_act "gelu"), fp32 arithmetic, erf by Abramowitz & Stegun 7.1.26
 *   (|error| <= 1.5e-7): the framework's fp16 result or its neighbour; within 1e-6 absolutely where the result underflows. */
int rdx_enc_gelu_f16(int device, void* x, int64_t n, void* stream);
/* rdx_enc_linear_small_f16: out[n_tokens][n_out] = act(x[n_tokens][n_in] w[n_out][n_in]^T + bias[n_out]) for at most 256 tokens (one
 *   question, a question's sub-queries): the weight matrix is read once, fp32 accumulation; act 0 = none, 1 = erf GELU (the
 *   checkpoint's). n_out a multiple of 16, n_in of 512. Larger token counts belong to the BLAS library. */
int rdx_enc_linear_small_f16(int device, const void* x, const void* w, const void* bias, int n_tokens, int n_out,
                             int n_in, int act, void* out, void* stream);

/* The forward of ONE question — `EmbeddingProvider.embed_query` / `embed([q])` in front of every `collection.query`
 * (reference src/utils/embedding_provider.py:118-157, called at src/rag/retriever.py:150-154, 212, 377) — as five launches per
 * transformer layer for at most 32 packed tokens (a question, or a question's short sub-queries). All pointers fp16 device
 * memory, 16-byte aligned, enqueued on `stream`, nothing synchronised. rag_dpo_amd/embedding_provider.py chains them and replays
 * the chain as one HIP graph.
 *
 * rdx_enc_embed_f16: out[t] = (word[tok[t]] + pos[pos_id[t]]) + type0 — the embedding sum in the module's order of fp16 adds; its
 *   LayerNorm is the first rdx_enc_stage_f16's prologue.
 * rdx_enc_stage_f16: out[n_tokens][n_out] = epi(in[n_tokens][n_in] w[n_out][n_in]^T + bias), fp32 accumulation, the weight matrix
 *   read once by n_out / features_per_workgroup workgroups (16, or 8 / 4 so that a 1024-feature projection still covers 128 / 256
 *   CUs; 0 = 16). n_in 512, 1024, 2048 or 4096.
 *     ln_gamma != NULL: `x` holds pre-LayerNorm sums s and in = LayerNorm(s) * ln_gamma + ln_beta (fp32 statistics, biased
 *       variance), recomputed by every workgroup; if y_out != NULL that LayerNorm output [n_tokens][n_in] is stored as well (the
 *       residual of the block's second half). n_in 512 or 1024, 16 features per workgroup, epilogue 0 or 1.
 *     ln_gamma == NULL: in = x, or rows x_rows[t] of x (and of `res`) when x_rows != NULL (the last layer: CLS rows only).
 *     epilogue 0: + bias; 1: erf GELU(+ bias); 2: res + (fp16)(+ bias) — the block's residual sum, rounded as the module's
 *       fp16 add rounds it; `out` then holds the next LayerNorm's input.
 * rdx_enc_attention_small_f16: rdx_enc_attention_f16 for at most 32 tokens on MFMA, one workgroup per head: token t attends to
 *   the tokens u with tok_first[u] == tok_first[t].
 * rdx_enc_layernorm_rows_f16: out[r] (fp32) = (fp16) LayerNorm(s[r]) — the last LayerNorm, on the CLS rows. */
int rdx_enc_embed_f16(int device, const int64_t* tok, const int64_t* pos_id, const void* word, const void* pos,
                      const void* type0, int n_tokens, int hidden, void* out, void* stream);
int rdx_enc_stage_f16(int device, const void* x, const int64_t* x_rows, const void* ln_gamma, const void* ln_beta,
                      float ln_eps, void* y_out, const void* w, const void* bias, const void* res, int n_tokens,
                      int n_out, int n_in, int epilogue, int features_per_workgroup, void* out, void* stream);
int rdx_enc_attention_small_f16(int device, const void* qkv, const int32_t* tok_first, int n_tokens, int heads,
                                int head_dim, float scale, void* ctx, void* stream);
int rdx_enc_layernorm_rows_f16(int device, const void* s, const void* gamma, const void* beta, float eps, int rows,
                               int hidden, float* out, void* stream);

/* The projections of a BATCH (any token count) with the epilogue the encoder applies next, and the LayerNorm that follows the residual
 * epilogue. fp16 device pointers, 16-byte aligned; `out` overlaps no input; enqueued on `stream`, nothing is synchronised or
 * allocated (graph-capturable). Arguments are validated before the device is touched.
 *
 * rdx_enc_gemm_f16: out[n_tokens][n_out] = epi(x[n_tokens][n_in] w[n_out][n_in]^T + bias[n_out]) on v_mfma_f32_16x16x32_f16, fp32
 *   accumulation in k order, w in the checkpoint's own layout (no re-tiled copy). n_tokens >= 0 is arbitrary (0: nothing is
 *   launched); n_out and n_in are multiples of 64. epilogue 0: + bias; 1: erf GELU(+ bias) in fp32 (rdx_enc_gelu_f16's erf);
 *   2: res[n_tokens][n_out] + (fp16)(+ bias), rdx_enc_stage_f16's residual epilogue (`res` is read for epilogue 2 only). No row at
 *   or past n_tokens of x, res or out is touched. No split-K, no atomics: the same inputs give the same bits on every call.
 *   At most 2^24 - 1 tiles (128 x 128 from 256 tiles on, else 64 x 64) per call.
 * rdx_enc_layernorm_f16: out[r] = LayerNorm(s[r]) * gamma + beta, fp16 in and out: rdx_enc_add_layernorm_f16 (same hidden sizes,
 *   statistics and rounding) for a sum that already exists; rows <= 4 * (2^24 - 1). */
int rdx_enc_gemm_f16(int device, const void* x, const void* w, const void* bias, const void* res, int64_t n_tokens,
                     int n_out, int n_in, int epilogue, void* out, void* stream);
int rdx_enc_layernorm_f16(int device, const void* s, const void* gamma, const void* beta, float eps, int64_t rows,
                          int hidden, void* out, void* stream);

/* Cross-encoder reranker --------------------------------------------------------------------- */
/* The stage the reference runs on every question between retrieval and generation: CrossEncoderReranker.rerank
 * (src/rag/reranker.py:112-216, called from src/rag/pipeline.py:221-262) — sentence-transformers' CrossEncoder.predict on the
 * (question, chunk) pairs, the topic boost, a stable sort and the min_score / keep-3 filter. rag_dpo_amd/reranker.py runs the
 * transformer backbone and calls these two on the pairs' <s> rows. Device pointers, enqueued on `stream`, nothing synchronised,
 * no allocation (both can be captured in a graph); no float atomics: the same inputs give bit-identical outputs on every call.
 *
 * rdx_rerank_head_f16: the XLMRobertaForSequenceClassification head with num_labels = 1, then a sigmoid:
 *     scores[p] = 1 / (1 + exp(-(w_out . tanh(w_dense cls[p] + b_dense) + b_out)))
 *   cls fp32 [n][hidden] (16-byte aligned), w_dense fp16 [hidden][hidden] (row = output feature, 16-byte aligned), b_dense and
 *   w_out fp16 [hidden], b_out fp16 [1], scores fp32 [n]. 1 <= n <= 1024, hidden a multiple of 64 in [64, 4096].
 *   workspace: RDX_RERANK_WORKSPACE_BYTES(n, hidden) bytes of device memory (8-byte aligned), scratch owned by the caller: the
 *   per-workgroup partial logits, summed in a fixed order by a second launch. Arithmetic: each z = w_dense cls + b_dense in fp32
 *   (fma in a fixed order), tanh, the w_out products, the logit sum and the sigmoid in fp64, the score rounded once to fp32.
 * rdx_rerank_select: final[p] = (double)scores[p], plus boosts[p] when boosts != NULL and boosts[p] > 0 (one fp64 add);
 *   order int32 [n] = the candidates by final descending, ties in input order (Python's stable sort(reverse=True); NaN last);
 *   final_score fp64 [n] in input order; *count = min(top_k, #{final >= min_score}), or keep_min when that is smaller and
 *   n >= keep_min (the reference keeps 3 even when top_k < 3). The reranked result is order[0 .. *count). 1 <= n <= 1024,
 *   top_k >= 0, keep_min >= 0. scores need not come from rdx_rerank_head_f16. */
#define RDX_RERANK_WORKSPACE_BYTES(n, hidden) ((size_t)((hidden) / 8) * (size_t)(n) * 8u)
int rdx_rerank_head_f16(int device, const float* cls, int n, int hidden, const void* w_dense, const void* b_dense,
                        const void* w_out, const void* b_out, double* workspace, float* scores, void* stream);
int rdx_rerank_select(int device, const float* scores, const double* boosts, int n, int top_k, double min_score,
                      int keep_min, int32_t* order, double* final_score, int32_t* count, void* stream);

/* Topic boost ---------------------------------------------------------------------------------- */
/* The `boosts` of rdx_rerank_select for all candidates of a question: the reference's TopicMatcher.topic_boost
 * (src/utils/rgpd_topics.py:178-222, called per candidate at src/rag/reranker.py:168-176). rag_dpo_amd/topics.py keeps the strings and
 * the embedding table and builds the inputs. Device pointers, enqueued on `stream`, nothing synchronised, no allocation, no float
 * atomics: the same inputs give bit-identical outputs on every call.
 *   table        fp32 [table_rows][dim] embeddings (unit rows for a cosine), 1 <= dim <= 4096, 4-byte aligned; may be NULL when
 *                table_rows = 0
 *   topic_slots  int32 [n_topics <= 32]: the table row of each question topic, in the question's order (repeats allowed)
 *   tag_slots    int32 [n_tags <= 65536]: the table rows of the call's distinct tags
 *                a slot that is negative or >= table_rows has no embedding: its similarities are exactly +0.0
 *   pair_offsets int32 [n + 1], pairs int32 [n_pairs]: candidate c owns the words pairs[pair_offsets[c] .. pair_offsets[c + 1]), each
 *                RDX_TOPIC_PAIR(topic index, tag index, exact), in the order of the reference's two loops (topics outer, the
 *                candidate's tags inner; at most 64 tags per candidate). exact = 1: the two strings are equal ignoring case.
 *   sims         fp64 [n_topics][n_tags] workspace owned by the caller (may be NULL when n_topics * n_tags = 0):
 *                sims[t][u] = sum_i (double)table[topic][i] * (double)table[tag][i], each product exact, added in a fixed order:
 *                64 partial sums (partial l takes i = l, l + 64, ... in that order, from +0.0) combined by a xor butterfly
 *                (s[l] += s[l ^ m] for m = 32, 16, 8, 4, 2, 1).
 *   boosts       fp64 [n], every entry written: best = 0.0; the pairs in order: an exact pair sets best = 1.0 and ends; a change of
 *                topic index with best >= 1.0 ends; otherwise best = sim when sim > best (never for a NaN or a negative sim).
 *                boosts[c] = +0.0 when best < threshold, else max_boost * (best - threshold) / (1.0 - threshold) in fp64.
 *   best_sim     NULL, or fp64 [n]: that best.
 * 1 <= n <= 1024. */
#define RDX_TOPIC_PAIR(topic, tag, exact) ((int32_t)(((uint32_t)(tag) << 8) | ((exact) ? 128u : 0u) | ((uint32_t)(topic) & 31u)))
int rdx_topic_boost(int device, const float* table, int64_t table_rows, int dim, const int32_t* topic_slots, int n_topics,
                    const int32_t* tag_slots, int n_tags, const int32_t* pair_offsets, const int32_t* pairs, int64_t n_pairs,
                    int n, double threshold, double max_boost, double* sims, double* boosts, double* best_sim, void* stream);

/* The reranker for a batch of questions ---------------------------------------------------------- */
/* The three calls above for nq questions at once (rag_dpo_amd/reranker.py rerank_batch). The candidates of all
 * questions lie side by side on one axis of n_total entries; question q is the segment [cand_off[q], cand_off[q + 1]). Enqueued on
 * `stream`, nothing synchronised, nothing allocated, no float atomics: the same inputs give the same bits on every call. Invalid
 * arguments return RDX_ERR_INVALID before anything is launched. Per question every output holds the bits and integers the
 * single-question call gives on that question alone; no question's result depends on its neighbours or on nq.
 *
 * Shape arrays. cand_off (and rdx_topic_boost_batch's topic_off, tag_off, sim_off) say where each question's data lies. The library
 * reads them on the host, to check the call and size the launches, and the kernels read the same words: they must lie in PINNED
 * HOST memory (hipHostMalloc / hipHostRegister; torch's pin_memory()) and stay unchanged until `stream` has passed the call. A
 * shape array in device or pageable memory is RDX_ERR_INVALID. Every other pointer is device memory.
 *   cand_off int32 [nq + 1]: cand_off[0] = 0, never decreasing, empty segments allowed, at most 1024 candidates per segment,
 *   n_total = cand_off[nq] <= RDX_RERANK_BATCH_MAX_ROWS; 1 <= nq <= RDX_RERANK_BATCH_MAX_QUESTIONS.
 *
 * rdx_rerank_head_rows_f16: rdx_rerank_head_f16 for 1 <= n <= RDX_RERANK_BATCH_MAX_ROWS rows (it knows no segments). scores[p] has
 *   the bits rdx_rerank_head_f16 gives row p in any call that contains it: a row's arithmetic does not depend on n. workspace:
 *   RDX_RERANK_WORKSPACE_BYTES(n, hidden) bytes.
 * rdx_topic_boost_batch: rdx_topic_boost per question over one shared table, two launches in all. Question q's topics are
 *   topic_slots[topic_off[q] .. topic_off[q + 1]) (at most 32), its distinct tags tag_slots[tag_off[q] .. tag_off[q + 1]) (at most
 *   65536), its similarity block sims + sim_off[q], [T_q][U_q] (sim_off int64 [nq + 1], sim_off[q + 1] - sim_off[q] >= T_q * U_q);
 *   candidate c of the axis owns pairs[pair_off[c] .. pair_off[c + 1]) (pair_off int64 [n_total + 1], device memory, clamped to
 *   [0, n_pairs]), RDX_TOPIC_PAIR words whose indices are local to the candidate's question. boosts fp64 [n_total], every entry
 *   written; best_sim NULL or fp64 [n_total]. A question without topics or without tags gets +0.0 boosts unless a pair is exact.
 * rdx_rerank_select_batch: rdx_rerank_select per segment in one launch. order int32 [n_total]: segment q's permutation, indices
 *   local to the segment, at order + cand_off[q]; final_score fp64 [n_total]; count int32 [nq] (0 for an empty segment); boosted
 *   NULL or int32 [nq]: the candidates of the segment with boosts > 0. One workgroup per question, RDX_RERANK_SELECT_WIDTHS
 *   threads wide: the smallest width that holds the call's longest segment. */
#define RDX_RERANK_BATCH_MAX_ROWS (1 << 20)
#define RDX_RERANK_BATCH_MAX_QUESTIONS 65535
#define RDX_RERANK_SELECT_WIDTHS {64, 256, 1024}
int rdx_rerank_head_rows_f16(int device, const float* cls, int64_t n, int hidden, const void* w_dense, const void* b_dense,
                             const void* w_out, const void* b_out, double* workspace, float* scores, void* stream);
int rdx_topic_boost_batch(int device, const float* table, int64_t table_rows, int dim, int nq, const int32_t* topic_off,
                          const int32_t* topic_slots, const int32_t* tag_off, const int32_t* tag_slots, const int64_t* sim_off,
                          const int32_t* cand_off, const int64_t* pair_off, const int32_t* pairs, int64_t n_pairs, double threshold,
                          double max_boost, double* sims, double* boosts, double* best_sim, void* stream);
int rdx_rerank_select_batch(int device, const float* scores, const double* boosts, int nq, const int32_t* cand_off, int top_k,
                            double min_score, int keep_min, int32_t* order, double* final_score, int32_t* count, int32_t* boosted,
                            void* stream);

/* Late-interaction rerank (MaxSim) ---------------------------------------------------------------- */
/* BGE-M3's third output, one vector per token, scored ColBERT-style (rag_dpo_amd/late_interaction.py):
 *     score(q, d) = (1 / n_q) * sum_i max_j q_i . d_j
 * over fp16 token vectors as stored. A dot product is accumulated in fp32 by v_mfma_f32_32x32x16_f16 in a fixed k order; the maximum
 * over the slot's tokens is exact; the n_q maxima are added in fp64 in token order, divided by n_q and rounded once to fp32.
 *   q_vecs fp16 [q_off[nq]][dim]: question q's token vectors are rows [q_off[q], q_off[q + 1]). q_off int32 [nq + 1] is a shape array
 *     (the rule above: PINNED HOST memory, read by the library to check the call and by the kernel; device or pageable memory is
 *     RDX_ERR_INVALID): q_off[0] >= 0, 1 to RDX_MAXSIM_MAX_Q_TOKENS rows per question, 1 <= nq <= RDX_RERANK_BATCH_MAX_QUESTIONS.
 *   d_vecs fp16 [d_rows][dim]: the arena. Slot s is rows [slot_start[s], slot_start[s] + slot_len[s]), 1 to RDX_MAXSIM_MAX_SLOT_TOKENS
 *     of them; slot_start int64 [n_slots], slot_len int32 [n_slots].
 *   Pair p scores question pair_q[p] (int32) against slot pair_slot[p] (int64) into scores[p] (fp32), 1 <= n_pairs <=
 *     RDX_MAXSIM_MAX_PAIRS; nothing behind scores[n_pairs - 1] is written. dim: a multiple of 32 in [32, RDX_MAXSIM_MAX_DIM].
 *   q_vecs and d_vecs are 16-byte aligned. Everything but q_off is device memory.
 * Invalid scalars or an invalid q_off return RDX_ERR_INVALID before anything is launched. A pair whose question or slot index is out
 * of range, or whose slot does not lie inside [0, d_rows) with an admitted length, gets NaN and reads nothing outside the arrays; its
 * neighbours are unaffected. No load leaves a pair's slot or its question's rows (a slot may end at the arena's last row). Enqueued on
 * `stream`, nothing synchronised, nothing allocated, no float atomics; a pair's bits do not depend on its position, on n_pairs or on
 * the other pairs of the call. One workgroup of four waves per pair (csrc/maxsim_kernel.hpp). */
#define RDX_MAXSIM_MAX_Q_TOKENS 256
#define RDX_MAXSIM_MAX_SLOT_TOKENS 8192
#define RDX_MAXSIM_MAX_DIM 1024
#define RDX_MAXSIM_MAX_PAIRS (1 << 20)
int rdx_maxsim_f16(int device, const void* q_vecs, const int32_t* q_off, int nq, const void* d_vecs, int64_t d_rows,
                   const int64_t* slot_start, const int32_t* slot_len, int64_t n_slots, const int32_t* pair_q,
                   const int64_t* pair_slot, int64_t n_pairs, int dim, float* scores, void* stream);

/* The same score over per-token symmetric int8 token vectors (rag_dpo_amd/late_interaction.py quantize_model / maxsim_i8_model,
 * DESIGN.md §32): half the bytes of a stored token, and a score that is the numpy model's bit for bit.
 *
 * rdx_maxsim_quantize_i8. vecs_f16 fp16 [rows][dim] -> codes int8 [rows][dim], scales fp32 [rows], per row:
 *     a = max_k |x_k|, scale = (float)((double)a / 127.0), c_k = clamp(rint((double)x_k / (double)scale), -127, 127)
 *   (fp64 divisions, ties to even). A row of zeros, or one holding NaN or Inf, gets codes 0 and scale +0.0. rows >= 1; dim: a multiple
 *   of 32 in [32, RDX_MAXSIM_MAX_DIM]. vecs_f16 and codes are 16-byte aligned device memory; nothing behind codes[rows * dim - 1] or
 *   scales[rows - 1] is written. One wave per row (csrc/maxsim_i8_kernel.hpp k_maxsim_quant).
 *
 * rdx_maxsim_i8. rdx_maxsim_f16's arguments with (q_codes, q_scales) and (d_codes, d_scales) in place of q_vecs and d_vecs: codes int8
 *   [rows][dim] (16-byte aligned), scales fp32 [rows], as rdx_maxsim_quantize_i8 writes them (scales finite and >= 0, +0.0 only for a row
 *   of zero codes, codes in [-127, 127]).
 *     acc_ij = sum_k cq_ik cd_jk  (int32, exact: v_mfma_i32_32x32x32_i8),  v_ij = (float)acc_ij * sd_j  (one fp32 multiply),
 *     m_i = max_j v_ij,  score = (float)((sum_i (double)sq_i * (double)m_i) / n_q)  (fp64, token order from +0.0).
 *   The limits, the q_off shape-array rule (PINNED HOST memory), the refusals, the NaN of an out-of-range pair, and what is read and
 *   written are rdx_maxsim_f16's. One workgroup of four waves per pair (csrc/maxsim_i8_kernel.hpp k_maxsim_i8).
 * Both are enqueued on `stream`, allocate nothing, synchronise nothing and use no atomics; an element's bits do not depend on its
 * position, on the call's length or on its neighbours. */
int rdx_maxsim_quantize_i8(int device, const void* vecs_f16, int64_t rows, int dim, int8_t* codes, float* scales, void* stream);
int rdx_maxsim_i8(int device, const int8_t* q_codes, const float* q_scales, const int32_t* q_off, int nq,
                  const int8_t* d_codes, const float* d_scales, int64_t d_rows,
                  const int64_t* slot_start, const int32_t* slot_len, int64_t n_slots,
                  const int32_t* pair_q, const int64_t* pair_slot, int64_t n_pairs, int dim, float* scores, void* stream);

/* `collection.query(query_embeddings=, n_results=k, where=)` (reference
 * src/rag/retriever.py:215-220,380-385; create_chromadb_index.py:405-408,435-439).
 *   queries     [nq][dim] raw fp32 (normalised on the device like corpus rows)
 *   allow_bits  NULL, or ceil(count/32) words: bit (r&31) of word r>>5 set = row r may be
 *               returned (the `where` pre-filter and tombstones, evaluated by the host layer)
 *   out_score   [nq][k] fp32 cosine, out_row [nq][k] int64 row ids, out_count [nq] number of valid
 *               entries (= min(k, allowed rows)); unused tail entries are (-inf, -1). */
int rdx_search(rdx_index* h, const float* queries, int64_t nq, int k, const uint32_t* allow_bits,
               float* out_score, int64_t* out_row, int32_t* out_count, int space, void* stream);

/* Resident `where` bitmaps. The reference's filters are a handful of fixed shapes (src/rag/pipeline.py:35-71,
 * pages/1_Chat.py:245-247) sent with every question: the host layer evaluates one ONCE, keeps the bitmap in HBM as an
 * rdx_mask and passes the handle with every search instead of re-uploading count/8 bytes. allow_bits as in rdx_search
 * (ceil(count/32) words, host or device). A mask belongs to the row count it was made for: any add / compact makes
 * rdx_search_masked refuse it (RDX_ERR_STATE) — rebuild it (update of a row's vector does not change the count; the host
 * layer drops its masks on every write anyway). mask == NULL = no filter. */
typedef struct rdx_mask rdx_mask;
int rdx_mask_create(rdx_index* h, const uint32_t* allow_bits, int space, rdx_mask** out);
int rdx_mask_destroy(rdx_mask* m);
int rdx_search_masked(rdx_index* h, const float* queries, int64_t nq, int k, const rdx_mask* mask, float* out_score,
                      int64_t* out_row, int32_t* out_count, int space, void* stream);

/* One search, a filter per query: a batch of questions from different users, each with the `where` the reference builds per user
 * (src/rag/pipeline.py:35-71) and hands to collection.query (src/rag/retriever.py:380-385), scanned in ONE pass over the corpus
 * instead of one rdx_search_masked per distinct filter.
 *   filters       host array of n_filters resident masks of this index, 0 <= n_filters <= 65535
 *   query_filter  host int32 [nq]: query q is held to filters[query_filter[q]], to no filter when query_filter[q] == -1. Equal entries
 *                 share a mask; a mask of zeros is valid (count 0).
 * Queries and outputs lie in `space`, as for rdx_search_masked; nq, k and the options follow rdx_search. Query q's scores, rows, count
 * and (-inf, -1) padding are, bit for bit, what rdx_search_masked returns for that query alone with its mask (NULL for -1): no query's
 * result depends on its neighbours, on nq, on the number of masks or on the path the search takes. The library uploads the masks'
 * device pointers and the indices into scratch of the index; more than 4096 queries are searched in chunks of 4096, each with its
 * slice of query_filter. When every query names the same mask, or none does, the call IS rdx_search_masked with that mask (NULL).
 * Otherwise the scan runs on the fp16 MFMA kernels or the exact path with a filter per query; the int8 coarse pass knows one bitmap
 * only and is not taken (planned with coarse_i8 = 0 whatever the option says: rdx_search_last_coarse_bits reports 16 or 0), and the
 * 256-query main scan runs its stand-alone emit check (no fused variant) with plain loads.
 * RDX_ERR_INVALID, before anything is enqueued and with the outputs untouched (the message names the query and the value): an entry
 * of query_filter outside [-1, n_filters); filters NULL with n_filters > 0, or a NULL handle in it; query_filter NULL with nq > 0;
 * n_filters outside [0, 65535]. A mask made for another row count or device: RDX_ERR_STATE, as for rdx_search_masked. */
int rdx_search_filtered(rdx_index* h, const float* queries, int64_t nq, int k, const rdx_mask* const* filters, int32_t n_filters,
                        const int32_t* query_filter, float* out_score, int64_t* out_row, int32_t* out_count, int space, void* stream);

/* The search in two halves, for callers that enqueue consumers of the results on the same stream (the multi-GPU path: the
 * RCCL all-gather of the partial top-k and the merge, reference has no counterpart). rdx_search_async enqueues the whole
 * search (device pointers only, nq <= 4096; mask may be NULL) and returns without waiting; rdx_search_wait blocks until that
 * search — not the stream: work enqueued behind it, e.g. the next batch's query encode, is not waited for — has completed and
 * runs its host half: when some queries' candidate segments overflowed (rare: clustered corpora) it
 * re-runs them through the fallback passes, synchronises the stream and reports *redone = 1 — results written by the first
 * pass were incomplete for those queries, so whatever consumed them on the stream must be re-enqueued. Any other call on
 * the index completes a pending search first. rdx_search == rdx_search_async + rdx_search_wait for device callers.
 * Lifetimes: `queries` is consumed by the kernels rdx_search_async enqueues (the fallback passes work from the index's own
 * normalised copy), so the caller may overwrite or free it with any STREAM-ORDERED work enqueued afterwards; the three output
 * buffers and out_flags must stay valid until rdx_search_wait has returned (the host half may rewrite them).
 * out_flags: NULL, or int32[RDX_PACKED_FLAGS] on the device. The search's last kernel stores out_flags[0] = 1 when the
 * results are incomplete and rdx_search_wait WILL redo them (exactly the cases in which it reports *redone = 1), else 0;
 * [1..3] = 0. rdx_search_wait stores 0 again once the fallback passes are enqueued: a consumer ordered after it sees
 * "complete". With the partial laid out as below the word travels with the all-gather, and every rank learns from the
 * merge (rdx_signal) whether ANY rank's partial was incomplete — no second collective, no device-to-host copy per step. */
#define RDX_PACKED_FLAGS 4
int rdx_search_async(rdx_index* h, const float* queries, int64_t nq, int k, const rdx_mask* mask, float* out_score,
                     int64_t* out_row, int32_t* out_count, int32_t* out_flags, void* stream);
int rdx_search_wait(rdx_index* h, int* redone);

/* Multi-GPU exchange step: merge n_parts per-shard partial results (after the RCCL all-gather,
 * SURVEY.md §8e) into the global top-k with the same ordering rule. Layouts:
 * part_score/part_row [n_parts][nq][k], part_count [n_parts][nq]; row ids must already be global (no row in two parts).
 * n_parts <= 64, k <= 4096; when n_parts * k exceeds 4096 the parts are folded pairwise (same result, more launches). */
int rdx_merge_topk(int device, const float* part_score, const int64_t* part_row,
                   const int32_t* part_count, int n_parts, int64_t nq, int k, float* out_score,
                   int64_t* out_row, int32_t* out_count, int space, void* stream);

/* A word in pinned host memory that a kernel publishes and the host waits on (spin, then stream synchronise): how the
 * merge tells the host whether any rank's partial carried the "incomplete" flag. One signal serves one stream of merges. */
typedef struct rdx_signal rdx_signal;
int rdx_signal_create(int device, rdx_signal** out);
int rdx_signal_destroy(rdx_signal* s);
/* blocks until the LAST rdx_merge_topk_packed given `s` has published; *value = OR over the parts of flags[0]. `stream` = the
 * stream that merge was enqueued on: never synchronised (work enqueued behind the merge is not waited for) — the word is spun
 * on for ~0.4 ms, then polled between short sleeps, and the stream is only queried now and then to report a lost merge. */
int rdx_signal_wait(rdx_signal* s, void* stream, int32_t* value);

/* Same merge, reading the partials straight out of the all-gather receive buffer (device memory):
 * part p starts part_stride bytes (multiple of 16) after part p-1 and is one rank's packed contribution
 * rows int64[nq][k] | scores f32[nq][k] | counts int32[nq] | flags int32[RDX_PACKED_FLAGS]
 * (= nq*k*12 + nq*4 + 16 bytes). Outputs are device pointers; k >= 1; n_parts * k <= 4096 (unlike rdx_merge_topk the packed form
 * does not fold: rag_dpo_amd/sharded.py checks world * k before it enqueues anything, so no rank fails behind a collective). sig: NULL, or the signal through which the first block
 * publishes the OR of the parts' flags[0] as soon as it has read them (the decision "some partial was incomplete: exchange
 * again" does not wait for the merge itself). */
int rdx_merge_topk_packed(int device, const void* packed, int64_t part_stride, int n_parts, int64_t nq,
                          int k, float* out_score, int64_t* out_row, int32_t* out_count, rdx_signal* sig, void* stream);

/* Diagnostics of the last rdx_search on this index (valid after the stream has synchronised). */
typedef struct rdx_search_stats {
    int64_t nq, k, rows;
    int64_t sample_rows;      /* rows scanned by the threshold bootstrap pass */
    int64_t emitted;          /* candidates emitted by the main scan (sum over queries) */
    int64_t rescored;         /* candidates re-scored exactly (sum over queries) */
    int64_t exact_queries;    /* queries answered by the exact full scan (fallback / small path) */
    int32_t path;             /* 0 = MFMA scan + exact re-score, 1 = exact scan only */
    int32_t profiled;         /* 1 if the ms_* fields below were measured */
    float ms_normalize, ms_scan_sample, ms_tau, ms_scan_main, ms_refine, ms_exact, ms_total;
    int64_t scan_main_launch_rows, scan_main_launch_queries; /* units of the dominant kernel */
    int64_t retried_queries;  /* queries whose candidate segments overflowed and that got a second MFMA pass */
    float xcd_finish_spread_ms; /* main scan: last XCD's finish minus first XCD's finish (0 when not measured) */
    float xcd_share_min, xcd_share_max; /* smallest / largest XCD share of the tiles (1.0 = an eighth) used by that scan */
    float tau_rank;           /* rank of the sampled score the scan threshold was taken from: k = provable, < k = speculative (verified per query) */
} rdx_search_stats;
int rdx_search_last_stats(rdx_index* h, rdx_search_stats* out);
/* Which coarse pass the last rdx_search's main scan ran: 16 (fp16 MFMA), 8 (int8 MFMA, option "coarse_i8") or 0 (the exact
 * full scan alone). Both coarse passes give the same ids and score bits. */
int rdx_search_last_coarse_bits(rdx_index* h, int32_t* bits);

/* BM25 sparse retrieval ----------------------------------------------------------------------- */
/* The sparse half of the reference's hybrid retrieval: rank_bm25 0.2.2 BM25Okapi scores (k1 = 1.5, b = 0.75, epsilon = 0.25)
 * behind ChunkBM25Index.search / SummaryBM25Index.search (reference src/rag/bm25_index.py:126-168, :242-292), called from
 * RAGRetriever.retrieve / retrieve_candidates (src/rag/retriever.py:258-285, :417-452). rag_dpo_amd/bm25.py tokenises, builds the
 * arrays below and maps rows back to chunk ids. The index is immutable: to refresh, build a new one (the reference rebuilds too).
 * Scores are float64 and bit-identical to numpy's
 *     score = 0; for each query term id t, in order, duplicates kept:  score += idf[t] * ((tf * 2.5) / (tf + row_denom))
 * Result order per query: score descending, ties by ascending row; only rows with score > 0 (and, with a filter, whose group's
 * bit is set) are returned. */
typedef struct rdx_bm25 rdx_bm25; /* opaque: one BM25 index resident in one GPU's HBM */
/* All pointers are host pointers; they are copied. CSR by term: term t's postings are [post_off[t], post_off[t+1]), rows strictly
 * ascending and < n_rows, tf >= 1. idf[n_terms] = the floored idf; row_denom[n_rows] = k1 * ((1 - b) + (b * doc_len) / avgdl) > 0.
 * row_group[n_rows] in [0, n_groups): the interned document_path of the row (reference `doc_filter`), or NULL with n_groups = 0.
 * Serves BM25Okapi(corpus_tokens) in SummaryBM25Index.build / ChunkBM25Index.build_from_collection (bm25_index.py:124, :234). */
int rdx_bm25_create(int device, int64_t n_rows, int64_t n_terms, const int64_t* post_off, const int32_t* post_row,
                    const uint16_t* post_tf, const double* idf, const double* row_denom, const int32_t* row_group,
                    int32_t n_groups, rdx_bm25** out);
int rdx_bm25_destroy(rdx_bm25* h);
/* nq queries: query q's term ids are term_ids[term_offsets[q] .. term_offsets[q+1]) (term_offsets[0] = 0, at most 4096 per query,
 * each in [0, n_terms): checked before anything is enqueued). 1 <= k <= 4096. space must be RDX_HOST: every pointer is a host one.
 * allow_groups: NULL = no filter, else a bitset of (n_groups + 31) / 32 words, bit g = rows of group g may be returned.
 * Out: out_score f64 [nq][k], out_row int64 [nq][k], out_count [nq] = min(k, rows passing); slots after the count hold 0 and -1.
 * Runs on `stream` (NULL = the index's own stream) of the index's device and is complete on return. Serves get_scores + the score > 0 / doc_filter /
 * sort / [:top_k] of bm25_index.py:146-168, :265-292; nq > 1 is several such searches in one call. */
int rdx_bm25_search(rdx_bm25* h, const int64_t* term_offsets, const int32_t* term_ids, int64_t nq, int k,
                    const uint32_t* allow_groups, double* out_score, int64_t* out_row, int32_t* out_count, int space,
                    void* stream);
/* rdx_bm25_search with a filter per query: filter_sets is a table [n_filters][(n_groups + 31) / 32] of bitsets as allow_groups is
 * one, and query_filter[q] in [-1, n_filters) is the row of the table that filters query q, -1 = no filter. Equal entries share a
 * set; a set of zeros is valid (its queries return count 0); n_filters = 0 with every entry -1 is rdx_bm25_search(.., NULL, ..).
 * Query q's result is, bit for bit, what rdx_bm25_search returns for that query alone with that set. The table and query_filter
 * travel in the upload of the offsets and ids: still one upload, one download. RDX_ERR_INVALID before anything is enqueued (the
 * outputs are not written), the message naming the query and the value: an entry outside [-1, n_filters); n_filters > 0 on an index
 * created without groups; filter_sets NULL with n_filters > 0; query_filter NULL with nq > 0. Everything else as rdx_bm25_search.
 * Serves the doc_filter of ChunkBM25Index.search (bm25_index.py:265-292) for a batch of questions, each with its own summary
 * pre-filter (retriever.py:417-452). */
int rdx_bm25_search_filtered(rdx_bm25* h, const int64_t* term_offsets, const int32_t* term_ids, int64_t nq, int k,
                             const uint32_t* filter_sets, int32_t n_filters, const int32_t* query_filter, double* out_score,
                             int64_t* out_row, int32_t* out_count, int space, void* stream);

/* BGE-M3 lexical weights (learned-sparse retrieval) ---------------------------------------------- */
/* BGE-M3's sparse output (rag_dpo_amd/lexical.py states the definition once, in numpy): a text is a set of terms
 * (sub-word token id, fp16 weight), one per distinct id, and
 *     score(question, chunk) = 0.0, then for each question term t in ascending id that the chunk has too:
 *                              score = score + (double)wq[t] * (double)wd[t]
 * in float64. The product of two fp16 values is exact in float64, so only the order of the additions rounds, and it is fixed.
 *
 * rdx_lex_reduce: the tokens of n_texts texts -> their terms. tok int32 [n_tok] and w fp32 [n_tok] are device memory: text i's tokens are
 * [off[i], off[i + 1]); off int64 [n_texts + 1] is a shape array (the rule above: PINNED HOST memory, read by the library to check the
 * call and by the kernel; device or pageable memory is RDX_ERR_INVALID), off[0] >= 0, non-decreasing, off[n_texts] <= n_tok, 0 to
 * RDX_LEX_MAX_TOKENS tokens per text. The rule per token: the weight is rounded once to fp16, round to nearest even; the token is
 * dropped when the fp16 value is not finite and above 0, or when its id is one of skip_ids[0 .. n_skip) (host pointer, 0 <= n_skip <=
 * RDX_LEX_MAX_SKIP); of the tokens left, one entry per distinct id with the largest weight, ascending by id.
 * Out (device memory): text i's terms are out_tok int32 / out_w uint16 (fp16 bits) [off[i] .. off[i] + out_n[i]); nothing else of
 * [off[i], off[i + 1]) is written and nothing outside it; out_n int32 [n_texts]. A text with an id outside [0, vocab) gets out_n = -1
 * and writes nothing; its neighbours are unaffected. Invalid scalars or an invalid off return RDX_ERR_INVALID before anything is
 * launched. Enqueued on `stream`, nothing synchronised, nothing allocated, no float atomics; one workgroup per text
 * (csrc/lex_kernel.hpp); a text's output does not depend on its position or on the other texts of the call. */
#define RDX_LEX_MAX_TOKENS 8192
#define RDX_LEX_MAX_SKIP 8
int rdx_lex_reduce(int device, const int32_t* tok, const float* w, int64_t n_tok, const int64_t* off, int64_t n_texts, int vocab,
                   const int32_t* skip_ids, int n_skip, int32_t* out_tok, uint16_t* out_w, int32_t* out_n, void* stream);
typedef struct rdx_lex rdx_lex; /* opaque: one index of lexical weights resident in one GPU's HBM; immutable, rebuilt to refresh */
/* All pointers are host pointers; they are copied. CSR by term over the tokenizer's vocabulary (n_terms = 250 002 for BGE-M3): term
 * t's postings are [post_off[t], post_off[t+1]), post_off[0] = 0, rows strictly ascending and < n_rows (refused otherwise: a term
 * occurs at most once per row, which is what fixes the order of a row's additions), post_w the fp16 bits of the weight, finite and
 * above 0 (bits in [0x0001, 0x7BFF]; anything else is refused). row_group / n_groups as in rdx_bm25_create. 6 bytes per posting plus
 * 8 (n_terms + 1) for the offsets, the per-term tile directory and 4 n_rows for the groups. */
int rdx_lex_create(int device, int64_t n_rows, int64_t n_terms, const int64_t* post_off, const int32_t* post_row,
                   const uint16_t* post_w, const int32_t* row_group, int32_t n_groups, rdx_lex** out);
int rdx_lex_destroy(rdx_lex* h);
/* nq questions: question q's terms are term_ids / term_w [term_offsets[q] .. term_offsets[q+1]) (term_offsets[0] = 0), term_w the fp16
 * bits of the weights. The filters are rdx_bm25_search_filtered's: a table filter_sets [n_filters][(n_groups + 31) / 32] and
 * query_filter[q] in [-1, n_filters), -1 = no filter (query_filter is required when nq > 0; n_filters = 0 with every entry -1 is an
 * unfiltered search). Result per question: the rows with score > 0 whose group passes, score descending, ties by ascending row, the
 * first k. Out as rdx_bm25_search: out_score f64 [nq][k], out_row int64 [nq][k], out_count [nq]; slots after the count hold 0 and -1.
 * RDX_ERR_INVALID before anything is enqueued (the outputs are not written), the message naming the query and the value: term ids of
 * a question not strictly ascending, or outside [0, n_terms); a weight that is not finite and above 0; more than 4096 terms in a
 * question; k outside [1, 4096]; a query_filter entry outside [-1, n_filters); space other than RDX_HOST. A question without terms, or
 * whose terms have no postings, returns count 0. Runs on `stream` (NULL = the index's own stream) and is complete on return.
 * The scorer is rdx_bm25_search's with the question's weight in place of idf[t] and the posting's weight in place of the Okapi
 * quotient (csrc/bm25_kernel.hpp k_lex_score); the merge is the same kernel. */
int rdx_lex_search(rdx_lex* h, const int64_t* term_offsets, const int32_t* term_ids, const uint16_t* term_w, int64_t nq, int k,
                   const uint32_t* filter_sets, int32_t n_filters, const int32_t* query_filter, double* out_score, int64_t* out_row,
                   int32_t* out_count, int space, void* stream);
/* rdx_lex_score_pairs: the score above of NAMED (question, row) pairs. Questions as in rdx_lex_search, but term_ids int32
 * and term_w uint16 are DEVICE memory (what EmbeddingProvider.embed_lexical_device returns, without a trip to the host) and
 * term_offsets int64 [nq + 1] is a shape array (the rule above: PINNED HOST memory, read by the library to check the call and by the
 * kernel): term_offsets[0] >= 0, non-decreasing, at most 4096 terms per question. Pair p scores question pair_q[p] (int32) against row
 * pair_row[p] (int64) into out_score[p] (f64), all device memory. Per pair the row is looked up in every question term's postings (a
 * binary search, behind the term's tile directory when its postings span more than one tile of 4 096 rows) and the exact products are
 * added in ascending term id from +0.0: bit for bit the score rdx_lex_search returns for that (question, row), and +0.0 for a row it
 * would not list. NaN, the neighbours unaffected and nothing read through it: a pair whose question is outside [0, nq) or whose row is
 * outside [0, n_rows); every pair of a question whose ids are not strictly ascending or outside [0, n_terms), or which holds a weight
 * whose bits are outside [0x0001, 0x7BFF]. RDX_ERR_INVALID before anything is launched: nq outside [1, 65535], n_pairs outside
 * [1, 2^20], an invalid term_offsets, a null or misaligned pointer. Enqueued on `stream`, nothing synchronised, nothing allocated, no
 * float atomics; a pair's bits do not depend on its position, on n_pairs or on its neighbours. One wave per pair
 * (csrc/lex_pairs_kernel.hpp; the lookup: csrc/lex_find.hpp). */
int rdx_lex_score_pairs(rdx_lex* h, const int64_t* term_offsets, const int32_t* term_ids, const uint16_t* term_w, int64_t nq,
                        const int32_t* pair_q, const int64_t* pair_row, int64_t n_pairs, double* out_score, void* stream);

/* Building a BM25 index from text ----------------------------------------------------------- */
/* The tokenizer of the reference's indexes (tokenize_french, bm25_index.py:38-49) and the vocabulary and postings that
 * BM25Okapi(corpus_tokens) derives from its tokens (bm25_index.py:124, :234), on the GPU: rag_dpo_amd/bm25_build.py uploads the
 * texts, calls the entry points below, sorts the keys with torch and hands rdx_bm25_create the arrays the host build would have
 * made, bit for bit. The rule over UTF-8 bytes, the term table and its protocol: csrc/bm25_build_kernel.hpp.
 * Limits: rows of one build < 2^31, bytes of one row < 2^32, table_slots <= 2^31. One build uses one stream. */
typedef struct rdx_bm25_build rdx_bm25_build; /* opaque: the term table of one build, in one GPU's HBM */
/* table_slots: a power of two in [2, 2^31], 16 bytes each. hash_mask is ANDed onto a token's hash before its slot is chosen:
 * all ones in production; a few bits make every token probe from a few slots (tests of the probe chains). Complete on return.
 * Serves BM25Okapi(corpus_tokens) (bm25_index.py:124, :234): the `nd` dictionary of its _initialize. */
int rdx_bm25_build_create(int device, int64_t table_slots, uint64_t hash_mask, rdx_bm25_build** out);
int rdx_bm25_build_destroy(rdx_bm25_build* h);
/* Tokenises one batch of rows. text (DEVICE, text_bytes bytes): the rows' UTF-8 texts, one 0x00 byte after each; it must stay
 * alive and unchanged until the build is destroyed (a term's slot holds the address of one of its occurrences). row_off (HOST,
 * n_rows + 1): row r is text[row_off[r] .. row_off[r+1] - 1), row_off[0] = 0, row_off[n_rows] = text_bytes; checked before
 * anything is enqueued. row_base: the build's number of this batch's first row. Out (DEVICE): doc_len[n_rows] = kept tokens per
 * row; keys: row r's stretch starts at the sum of (len + 1) / 3 over the rows before it and holds (len + 1) / 3 entries: one
 * (slot << 32) | (row_base + r) per kept token, in any order, then -1. key_cap >= that sum over all rows. Asynchronous on
 * `stream`. Serves tokenize_french + BM25Okapi(corpus_tokens) (bm25_index.py:38-49, :124, :234). */
int rdx_bm25_build_tokenize(rdx_bm25_build* h, const uint8_t* text, int64_t text_bytes, const int64_t* row_off, int64_t n_rows,
                            int64_t row_base, int64_t* keys, int64_t key_cap, int32_t* doc_len, void* stream);
/* Waits for the batches enqueued so far. terms = occupied slots, tokens = kept tokens, full = 1 when more than half of the
 * slots were taken: tokens were then dropped and the build must start over with a larger table. Any of the three may be NULL.
 * Serves BM25Okapi(corpus_tokens) (bm25_index.py:124, :234): corpus_size and the vocabulary's size. */
int rdx_bm25_build_stats(rdx_bm25_build* h, int64_t* terms, int64_t* tokens, int32_t* full);
/* out_first_pos (DEVICE, n = table_slots): per slot (row << 32) | byte offset in the row of its term's first occurrence, or -1
 * for a free slot. The occupied slots sorted by it are the terms in first-occurrence order: the order in which
 * BM25Okapi(corpus_tokens) (bm25_index.py:124, :234) meets them, which fixes the order of its idf sum. Asynchronous on `stream`. */
int rdx_bm25_build_first_pos(rdx_bm25_build* h, int64_t* out_first_pos, int64_t n, void* stream);
/* The vocabulary. slots (DEVICE, n_terms): term t's slot. arena == NULL: term_off[t] = bytes of term t (n_terms entries). Else
 * term_off (DEVICE, n_terms + 1) holds the terms' offsets and term t's normalised UTF-8 bytes go to arena[term_off[t] ..
 * term_off[t+1]), never past arena_bytes. Asynchronous on `stream`. Serves the keys of BM25Okapi(corpus_tokens)'s idf dictionary
 * (bm25_index.py:124, :234), which get_scores looks query tokens up in. */
int rdx_bm25_build_vocab(rdx_bm25_build* h, const int32_t* slots, int64_t n_terms, int64_t* term_off, uint8_t* arena,
                         int64_t arena_bytes, void* stream);

/* Document store and where_document --------------------------------------------------------- */
/* Chroma's where_document filter (chromadb 1.x `get` / `query` / `delete`): {"$contains": s}, {"$not_contains": s}, and
 * {"$and": [...]} / {"$or": [...]} over them, nested to any depth; rag_dpo_amd/where_document.py validates the tree and compiles
 * it into the leaves and the postfix program below. Match rule: case-sensitive, byte-exact substring of the UTF-8 text (exactly
 * Python's `needle in document`, UTF-8 being self-synchronising). A row without text (len 0) contains nothing; $not_contains is
 * the complement of $contains, so such a row matches it; rows the caller has deleted are removed through base_bits.
 *
 * An rdx_docs holds the rows' text on one device, in the collection's row order. Layout: each row's bytes start on a 16-byte
 * boundary and are zero-padded to the next one; the row table is (start int64, len int32); the arena ends with at least 64 zero
 * bytes. The store is independent of an rdx_index (the host keeps the two in step: same rows, same compaction keep lists).
 *
 * Calls that change the store (append / replace / compact) and rdx_docs_set_query take host pointers only and are complete on
 * return; they first wait for the store's last filter / contains call to finish on its stream. The query is set by one host call
 * and run by rdx_docs_contains / rdx_docs_filter, whose `space` covers their own bitmap pointers: this split keeps the rule that
 * one `space` says where every pointer of a call lives (the patterns are validated and uploaded once, on the host, whatever
 * space the bitmaps live in). Arguments are validated before the store handle is used. */
typedef struct rdx_docs rdx_docs; /* opaque: one document store resident in one GPU's HBM */
#define RDX_DOCS_MAX_LEAVES 1024  /* patterns per query; the scan tests 32 per pass (LDS-staged, <= 256 bytes) */
#define RDX_DOCS_OP_NOT (-1)      /* program ops: >= 0 = push leaf i's bitmap; NOT / AND / OR on the top of the stack */
#define RDX_DOCS_OP_AND (-2)
#define RDX_DOCS_OP_OR (-3)
int rdx_docs_create(int device, rdx_docs** out);
int rdx_docs_destroy(rdx_docs* h);
/* appends n rows: row i's text is bytes[offsets[i] .. offsets[i+1]) (offsets[0] = 0, non-decreasing; a row < 2^31 - 64 bytes) */
int rdx_docs_append(rdx_docs* h, const uint8_t* bytes, const int64_t* offsets, int64_t n);
/* row_ids[i] gets the text bytes[offsets[i] .. offsets[i+1]): written at the arena tail, the old bytes become dead; the arena is
 * rewritten densely (the rows keep their ids) once dead bytes exceed both the live bytes and 16 MiB */
int rdx_docs_replace(rdx_docs* h, const int64_t* row_ids, const uint8_t* bytes, const int64_t* offsets, int64_t n);
/* keeps the rows keep[0 .. n_keep) (strictly ascending: the keep list of rdx_index_compact), renumbered 0 .. n_keep-1 */
int rdx_docs_compact(rdx_docs* h, const int64_t* keep, int64_t n_keep);
/* rows; live_bytes = padded bytes of the rows' current text; arena_bytes = padded bytes in use, dead text included */
int rdx_docs_stats(const rdx_docs* h, int64_t* rows, int64_t* live_bytes, int64_t* arena_bytes);
/* the query: P leaf patterns, leaf p = pat_bytes[pat_off[p] .. pat_off[p+1]) (pat_off[0] = 0, strictly increasing: no empty
 * pattern), 1 <= P <= RDX_DOCS_MAX_LEAVES, any length (patterns over 256 bytes take a slower kernel); program: n_ops postfix ops
 * (n_ops <= 4096, at most 16 stack entries, leaving exactly one; n_ops = 0: leaves only, for rdx_docs_contains) */
int rdx_docs_set_query(rdx_docs* h, const uint8_t* pat_bytes, const int64_t* pat_off, int P, const int32_t* program, int n_ops);
/* out_bits [P][ceil(rows/32)] words: bit (r&31) of word p*words + (r>>5) = row r contains leaf p; tail bits zero */
int rdx_docs_contains(rdx_docs* h, uint32_t* out_bits, int space, void* stream);
/* out_bits [ceil(rows/32)] = program(leaf bitmaps) AND base_bits (NULL = all rows), tail bits past `rows` zero: the allow_bits
 * of rdx_search / rdx_mask_create. RDX_DEVICE: enqueued on `stream`, nothing crosses PCIe. */
int rdx_docs_filter(rdx_docs* h, const uint32_t* base_bits, uint32_t* out_bits, int space, void* stream);

/* Metadata store and `where` -------------------------------------------------------------------- */
/* Chroma's `where` filter (`collection.query(where=...)`, reference src/rag/pipeline.py:35-71, pages/1_Chat.py:245-247) evaluated on
 * the device from metadata columns resident in HBM. rag_dpo_amd/where.py states the semantics and is the model;
 * rag_dpo_amd/where_device.py validates a filter and compiles it into the leaves and the postfix program below.
 *
 * An rdx_meta holds some of a collection's metadata columns on one device, in the collection's row order; a column lives in a
 * "slot" (0 <= col < RDX_META_MAX_COLUMNS) chosen by the caller. Layout per slot: kind uint8 [rows] (0 missing, 1 str, 2 int,
 * 3 float, 4 bool: where.py K_*) and payload double [rows] — the value of an int / float / bool row, (double)code of a str row
 * (code = the string's index in the column's host vocabulary, exact in a double), +0.0 for a missing row: 9 bytes per row. The
 * store is independent of an rdx_index (the host keeps the two in step) and allocates nothing on the device until rows are set.
 *
 * A leaf is true for a row iff the row's kind equals the leaf's kind and `payload <op> operand` holds as an IEEE double
 * comparison (the operand of a str leaf is its code, of any other leaf its num): a NaN operand matches nothing, -0.0 equals 0.0,
 * an int 1 matches neither a bool True nor a float 1.0, a missing row matches no leaf (where.py Column._eq / Column._cmp).
 * RDX_META_CONST0 / _CONST1 are false / true for every row and read no column (a key no row has).
 *
 * rdx_meta_set_rows / _drop_column / _truncate / _set_query take host pointers only and are complete on return; the ones that
 * write or free device memory (set_rows with n > 0, drop_column of a slot in use, set_query) first wait for the store's last
 * rdx_meta_filter to finish on its stream; truncate only lowers row counts and waits for nothing. Changing the store (the first three) unsets the query: call
 * rdx_meta_set_query again before the next rdx_meta_filter. Arguments are validated before the store handle is used and before
 * the device is touched. */
typedef struct rdx_meta rdx_meta; /* opaque: metadata columns resident in one GPU's HBM */
#define RDX_META_MAX_COLUMNS 4096
#define RDX_META_MAX_LEAVES 1024
#define RDX_META_EQ 0 /* leaf ops */
#define RDX_META_GT 1
#define RDX_META_GE 2
#define RDX_META_LT 3
#define RDX_META_LE 4
#define RDX_META_CONST0 5
#define RDX_META_CONST1 6
#define RDX_META_OP_NOT (-1) /* program ops: >= 0 = push leaf i's verdict; NOT / AND / OR on the top of the stack (= RDX_DOCS_OP_*) */
#define RDX_META_OP_AND (-2)
#define RDX_META_OP_OR (-3)
typedef struct rdx_meta_leaf {
    int32_t col;  /* column slot (ignored by CONST0 / CONST1) */
    int32_t op;   /* RDX_META_EQ .. RDX_META_CONST1 */
    int32_t kind; /* 1 str (op EQ only), 2 int, 3 float, 4 bool */
    int32_t code; /* operand of a str leaf; a code no row holds (e.g. -2: a string not in the vocabulary) matches nothing */
    double num;   /* operand of an int / float / bool leaf */
} rdx_meta_leaf;
int rdx_meta_create(int device, rdx_meta** out);
int rdx_meta_destroy(rdx_meta* h);
/* writes rows [first_row, first_row + n) of slot `col` from host arrays kind uint8 [n] (each <= 4), num double [n] (read for
 * int / float / bool rows), code int32 [n] (read for str rows). The column grows as needed; rows between its old end and
 * first_row become "missing". */
int rdx_meta_set_rows(rdx_meta* h, int col, int64_t first_row, const uint8_t* kind, const double* num, const int32_t* code,
                      int64_t n);
/* frees slot `col` (it then holds no rows) */
int rdx_meta_drop_column(rdx_meta* h, int col);
/* every column longer than `rows` is cut to `rows` rows (memory is kept) */
int rdx_meta_truncate(rdx_meta* h, int64_t rows);
/* columns = slots holding rows; bytes = device memory allocated for them (0 until the first rdx_meta_set_rows) */
int rdx_meta_stats(const rdx_meta* h, int64_t* columns, int64_t* bytes);
/* the query: 1 <= n_leaves <= RDX_META_MAX_LEAVES leaves and a postfix program of 1 <= n_ops <= 4096 ops using at most 16 stack
 * entries and leaving exactly one. A leaf (other than a CONST) naming a slot that holds no rows: RDX_ERR_INVALID. */
int rdx_meta_set_query(rdx_meta* h, const rdx_meta_leaf* leaves, int n_leaves, const int32_t* program, int n_ops);
/* out_bits [ceil(rows/32)] = program AND base_bits (NULL = all rows; the caller's tombstones), bits past `rows` zero: the
 * allow_bits of rdx_search / rdx_mask_create. `space` covers base_bits and out_bits. Every column the query names must hold
 * exactly `rows` rows and a query must be set, else RDX_ERR_STATE (nothing is launched). RDX_DEVICE: one kernel enqueued on
 * `stream`; nothing is synchronised or allocated and nothing crosses PCIe. RDX_HOST: complete on return. */
int rdx_meta_filter(rdx_meta* h, int64_t rows, const uint32_t* base_bits, uint32_t* out_bits, int space, void* stream);

/* Inner-product and squared-L2 spaces ------------------------------------------------------------ */
/* Chroma's two other spaces (`create_collection(metadata={"hnsw:space": "ip" | "l2"})`) on the cosine engine; DESIGN.md §17 has the
 * reduction and the proof, rag_dpo_amd/spaces.py drives these calls and is their model, bit for bit.
 *
 * The contract of such a collection. Stored embeddings are kept exactly as given (fp32; get / query return them bit for bit; nothing
 * is normalised). distance = 1 - sum_j q_j x_j (ip) or sum_j (q_j - x_j)^2 (l2: the SQUARED Euclidean distance), computed in fp64
 * from the raw fp32 query and the raw fp32 row in a fixed order — 64 partial sums, partial l takes j = l, l + 64, ... in that order
 * from +0.0, combined by the xor butterfly s[l] += s[l ^ m], m = 32, 16, 8, 4, 2, 1 (rdx_topic_boost's order) — and rounded to fp32
 * once. ip: the term is (double)q_j * (double)x_j and the distance (float)(1.0 - sum). l2: diff = (double)q_j - (double)x_j,
 * sq = diff * diff, acc += sq, each rounded, never fused. Result order per query: fp32 distance ascending, ties by ascending row
 * id; counts, padding (+inf, -1), filters and tombstones as in the cosine space. NaN / Inf are rejected; so is a row whose lifted
 * form is not finite or whose power-of-two scaling is not exactly invertible in fp32. Results depend on the raw values only.
 *
 * The engine rows ("lifted"): y = 2^e x (ip, engine dim = dim) or y = 2^e (x, a, 0, 0, 0) with a = (float)(-|x|^2 / 2), |x|^2 in the
 * order above (l2, engine dim = dim + 4; a query is (q, 1, 0, 0, 0)); e = scale_exp, one per collection, chosen so that every
 * |y| <= 1. They are stored with rdx_index_add_stored / rdx_index_update_stored; x = 2^-e y exactly.
 *
 * All four calls: device pointers, enqueued on `stream`, nothing synchronised, no allocation, no float atomics (the same inputs
 * give the same bits); arguments are validated before the device is touched. dim: the RAW dimension, a multiple of 4 with the
 * engine dimension at most 4096. Rows, queries and engine rows are 16-byte aligned.
 *
 * rdx_space_measure: lifted_sq[i] (fp64) = |x_i|^2 (ip) or |x_i|^2 + a_i^2 (l2), the squared norm of the lifted row before
 *   scaling; bad[i] = 1 when the row holds NaN / Inf or a_i is not finite, else 0. The host picks scale_exp from the largest.
 * rdx_space_lift: out [n][engine dim] from rows [n][dim] and scale_exp (is_query = 1: queries, scale_exp 0, fifth column 1);
 *   bad[i] = 1 when some element does not scale back to its own bits (ldexpf(ldexpf(x, e), -e) != x), else 0.
 * rdx_space_rescore: per query b the candidates cand_rows / cand_scores [nq][kp] (what rdx_search returned for the lifted query with
 *   k = kp; cand_counts [nq]) and their engine rows cand_vecs [nq][kp][engine dim] (rdx_index_get of cand_rows; slots past the
 *   count are not used) -> the k best by (distance, row): out_dist / out_row [nq][k], out_count [nq] = min(k, count), and
 *   out_proven [nq] = 1 when no row outside the candidates can belong to the answer: count < kp, or the lower bound on the
 *   distance of every other row — from the lowest candidate score plus `guard` (spaces.GUARD_IP / GUARD_L2) — is strictly above the k-th distance.
 *   work_dist: [nq][kp] floats of scratch owned by the caller. 1 <= k <= kp <= 4096, nq <= 65535.
 * rdx_space_distances: out[b * out_stride + r] = distance(query b, engine row r of the page vecs [n][engine dim]), or +inf when bit
 *   first_row + r of allow_bits (NULL = all rows) is clear: the brute-force pass. nq <= 64, n <= 2^24. */
#define RDX_SPACE_IP 0
#define RDX_SPACE_L2 1
int rdx_space_measure(int device, int space_kind, const float* rows, int64_t n, int dim, double* lifted_sq, int32_t* bad,
                      void* stream);
int rdx_space_lift(int device, int space_kind, int is_query, const float* rows, int64_t n, int dim, int scale_exp, float* out,
                   int32_t* bad, void* stream);
int rdx_space_rescore(int device, int space_kind, const float* queries, int64_t nq, int dim, const float* cand_vecs,
                      const int64_t* cand_rows, const float* cand_scores, const int32_t* cand_counts, int kp, int k,
                      int scale_exp, double guard, float* work_dist, float* out_dist, int64_t* out_row, int32_t* out_count,
                      int32_t* out_proven, void* stream);
int rdx_space_distances(int device, int space_kind, const float* queries, int nq, int dim, const float* vecs, int64_t n,
                        int scale_exp, const uint32_t* allow_bits, int64_t first_row, float* out, int64_t out_stride,
                        void* stream);

/* Rank fusion ----------------------------------------------------------------------------------- */
/* The step that joins the dense and the BM25 rankings of a question: the reference's summary filter of the dense lists, the
 * min-distance / max-score merge, reciprocal rank fusion, the stable sort and the cut (src/rag/retriever.py:226-300, :391-462), as
 * DenseRetriever._fuse (rag_dpo_amd/retriever.py) computes them — that method is the model, bit for bit — for nq questions in ONE
 * launch, one workgroup per question. rag_dpo_amd/fusion.py packs the lists and builds the winners' objects; DESIGN.md §18.
 *
 * Limits (RDX_ERR_INVALID beyond them, checked before anything is launched or written): 1 <= n_lists <= RDX_FUSE_MAX_LISTS lists per
 * question, 1 <= list_stride <= RDX_FUSE_MAX_LIST_ENTRIES entries per list, n_lists * list_stride <= RDX_FUSE_MAX_ENTRIES entries per
 * question, 1 <= top_n <= RDX_FUSE_MAX_ENTRIES, nq <= 2^24.
 *
 * Input. Question q's lists are [q][0 .. n_lists) in the order _fuse visits them (dense q0, BM25 q0, dense q1, BM25 q1, ...):
 *   list_kind   int32 [nq][n_lists]  RDX_FUSE_DENSE or RDX_FUSE_BM25
 *   list_weight fp64  [nq][n_lists]  the ranking's RRF weight
 *   list_count  int32 [nq][n_lists]  entries of the list, 0 .. list_stride; -1 = the list is absent (a skipped sub-query: no ranking,
 *                                    no weight). RDX_HOST: counts and kinds outside these values are RDX_ERR_INVALID; RDX_DEVICE (they
 *                                    cannot be read before the launch): a count above list_stride is read as list_stride, below -1 as -1.
 *   keys        int64 [nq][n_lists][list_stride]  what identifies a chunk across lists (the host layer: its collection row)
 *   dense_dist  fp32  [nq][n_lists][list_stride]  read for the entries of dense lists: the distance
 *   bm25_score  fp64  [nq][n_lists][list_stride]  read for the entries of BM25 lists: the score
 *   filter_on   NULL (no question is filtered), or int32 [nq]: != 0 = question q's dense lists are filtered by
 *   allow_groups uint32 [nq][group_words]: bit (g & 31) of word g >> 5 set = document group g is allowed, and
 *   row_group   int32 [n_rows]: the group of key r. A dense key that is negative, >= n_rows, or whose group is negative or
 *               >= 32 * group_words is never allowed.
 * Filtering. A dense list of a filtered question becomes its allowed entries, in order; when fewer than min_semantic are allowed, its
 *   first refused entries follow, in order, up to min_semantic entries in all. Every other list is taken as given.
 * Per key, over the filtered lists in list order, then rank order ("first appearance" = the first such occurrence):
 *   distance (fp32)  the first appearance's distance, or 1.0 when that is a BM25 one; then d wherever a later dense occurrence has d < distance
 *   semantic (fp64)  1.0 / (1.0 + (double)distance) of the first appearance, or +0.0 when that is a BM25 one; then the value s of a
 *                    later dense occurrence wherever s > semantic (the two are not functions of each other)
 *   bm25 (fp64)      +0.0, then over the BM25 occurrences: s where s > bm25 (bm25_keep_max = 1) or the last s (bm25_keep_max = 0)
 *   hybrid (fp64)    with more than one list present (count >= 0; an empty list counts): +0.0, then
 *                    += list_weight / (double)(rrf_k + rank + 1) at EVERY occurrence (rank = 0-based position in the filtered list;
 *                    IEEE division, one add each, in that order). With one list or none present: hybrid = semantic.
 * Output per question: the keys by hybrid descending, ties (+0.0 == -0.0) by first appearance — Python's stable sort(reverse=True) over
 *   dict insertion order; NaN after every number. out_count [nq] = min(top_n, distinct keys); [nq][top_n] each: out_key, out_distance,
 *   out_semantic, out_bm25, out_hybrid, and out_list / out_rank = the INPUT position (list, rank before filtering) of the key's first
 *   appearance: where the host takes the chunk's text and metadata from. Slots past the count hold key -1, list -1, rank -1 and zeros.
 * `space` covers every pointer. RDX_DEVICE: one launch enqueued on `stream`, nothing synchronised or allocated, no atomics — the same
 * inputs give the same bits on every call, whatever nq. RDX_HOST: staged through the device, complete on return (NULL = HIP's default stream). */
#define RDX_FUSE_MAX_LISTS 16
#define RDX_FUSE_MAX_LIST_ENTRIES 512
#define RDX_FUSE_MAX_ENTRIES 1024
#define RDX_FUSE_DENSE 0
#define RDX_FUSE_BM25 1
int rdx_fuse_rankings(int device, int64_t nq, int n_lists, int list_stride, const int32_t* list_kind, const double* list_weight,
                      const int32_t* list_count, const int64_t* keys, const float* dense_dist, const double* bm25_score,
                      const int32_t* row_group, int64_t n_rows, const int32_t* filter_on, const uint32_t* allow_groups,
                      int group_words, int min_semantic, int bm25_keep_max, int rrf_k, int top_n, int64_t* out_key,
                      float* out_distance, double* out_semantic, double* out_bm25, double* out_hybrid, int32_t* out_list,
                      int32_t* out_rank, int32_t* out_count, int space, void* stream);

/* Grouped search -------------------------------------------------------------------------------- */
/* Exact top-k grouped by a metadata key: the first n_want distinct groups met while walking a query's ranking (score descending, row
 * ascending), each with its first group_size rows. It replaces the reference's heuristic — fetch n_docs*10 chunks (src/rag/retriever.py:202)
 * and deduplicate them by document on the host (src/rag/retriever.py:539-578) — by the exact answer. rag_dpo_amd/groups.py drives the two
 * calls; DESIGN.md §21.
 *
 * rdx_group_select (serves retriever.py:539-578 over the n_docs*10 list of :202). Cuts ranked lists, as a search returned them, into groups:
 * one workgroup per query, independent of any index. Device pointers only, one launch enqueued on `stream`, nothing allocated or synchronised.
 *   scores fp32 / rows int64 [nq][k], counts int32 [nq]: the lists; entries at or beyond the count, and entries whose row is negative, are padding
 *   row_group int32 [n_rows]: a row's group code in [0, n_groups), or -1 = the row has no group and is ignored
 *   group_off int64 [n_groups + 1]: non-decreasing; group c has group_off[c + 1] - group_off[c] rows in the whole collection
 *   out_score fp32 / out_row int64 [nq][n_want][group_size]: the members in ranking order (padding -inf / -1)
 *   out_count / out_code / out_complete int32 [nq][n_want]: members written; the group's code (-1 past the groups found); 1 = the members
 *     are the group's first group_size rows of the WHOLE ranking (the list is not full, or it holds min(group_size, |group|) rows of the group)
 *   out_found / out_short int32 [nq]: groups written; 1 = the list is full (count == k) and holds fewer than n_want groups, so a longer
 *     list may hold more
 *   out_bad int32 [1], zeroed by the caller: set to 1 when a listed row is >= n_rows or its code is >= n_groups. Such an entry is treated
 *     as padding and nothing is read through it; the caller treats the call as failed.
 * Limits (RDX_ERR_INVALID, before anything is enqueued): nq <= 65535, 1 <= k <= RDX_GROUP_MAX_K, 1 <= n_want <= RDX_GROUP_MAX_GROUPS,
 * 1 <= group_size <= RDX_GROUP_MAX_SIZE, n_groups < 2^31.
 *
 * rdx_index_group_fill (serves the same reference call, for the groups whose rows the n_docs*10 list of :202 cut off). Job j: the best
 * group_size rows of group_rows[job_begin[j], job_end[j]) that `mask` allows (NULL: all), for query job_query[j], by (exact score descending,
 * row ascending) with the scores of rdx_search bit for bit (the same normalisation of `queries`, the same summation order).
 *   queries fp32 [nq][dim], group_rows int64 [n_group_rows], the outputs: device memory. job_query int32 / job_begin / job_end int64
 *   [n_jobs]: HOST memory, checked before anything is enqueued (0 <= job_query < nq, 0 <= begin <= end <= n_group_rows, a span of at most
 *   RDX_GROUP_FILL_SPAN rows: longer groups are split by the caller and the parts' lists merged). An entry of group_rows that is not a row
 *   of the index is skipped, never read. out_score fp32 / out_row int64 [n_jobs][group_size] (padding -inf / -1), out_count int32 [n_jobs].
 * Enqueued on `stream`; the call returns when the results are complete. RDX_ERR_STATE on an index with mapped row ids (a shard). */
#define RDX_GROUP_MAX_K 4096
#define RDX_GROUP_MAX_GROUPS 64
#define RDX_GROUP_MAX_SIZE 16
#define RDX_GROUP_FILL_SPAN 4096
int rdx_group_select(int device, const float* scores, const int64_t* rows, const int32_t* counts, int64_t nq, int k,
                     const int32_t* row_group, int64_t n_rows, const int64_t* group_off, int64_t n_groups, int n_want, int group_size,
                     float* out_score, int64_t* out_row, int32_t* out_count, int32_t* out_code, int32_t* out_complete,
                     int32_t* out_found, int32_t* out_short, int32_t* out_bad, void* stream);
int rdx_index_group_fill(rdx_index* h, const float* queries, int64_t nq, const rdx_mask* mask, const int32_t* job_query,
                         const int64_t* job_begin, const int64_t* job_end, int64_t n_jobs, const int64_t* group_rows,
                         int64_t n_group_rows, int m, float* out_score, int64_t* out_row, int32_t* out_count, void* stream);

/* Diversity-aware selection (MMR) --------------------------------------------------------------- */
/* Maximal marginal relevance over candidate lists, as a search returned them: what a user of the reference's store gets today only by
 * fetching more chunks than needed (src/rag/retriever.py:202) and deduplicating them on the host (:539-578), which cannot tell two
 * near-identical chunks of different documents apart. rag_dpo_amd/mmr.py states the definition and drives the call; DESIGN.md §22.
 *
 * rdx_index_mmr. Per query: the live entries of its list are those at a position below cand_count whose row is in [0, rows of the index).
 * Pick 0 is the first live position. Every later pick is the live unpicked position i with the largest
 *     v_i = lambda * (double)s_i - (1.0 - lambda) * (double)m_i        (three fp64 operations, each rounded once, never fused)
 * where s_i is the entry's score as given and m_i the largest fp32 pair score p(i, j) over the picked j; ties go to the smaller
 * position. p(i, j) is the exact score of rdx_search with the stored (normalised) row of j as the query and the row of i as the corpus
 * row: the same summation order, the same bits, and symmetric. min(k, live entries) picks are made.
 *   cand_score fp32 / cand_row int64 [nq][fetch_k], cand_count int32 [nq]: the lists (a count outside [0, fetch_k] is clamped). The scores
 *     of live entries must be finite. The lists need not be sorted; those of a search are, and then pick 0 is the best entry.
 *   out_pos int32 / out_row int64 / out_score fp32 / out_value double [nq][k], in pick order: the pick's position in its list, its row, its
 *     score as given and its v (pick 0: lambda * (double)s); padding -1 / -1 / -inf / -inf. out_count int32 [nq]: picks made.
 *   out_bad int32 [1], zeroed by the caller: set to 1 when a listed row is >= the index's rows. Such an entry is treated as padding and
 *     nothing is read through it; the caller treats the call as failed.
 * Device pointers only; one launch enqueued on `stream`, nothing allocated or synchronised; the same list gives the same bits whatever nq.
 * Limits (RDX_ERR_INVALID, before anything is enqueued): nq <= 65535, 1 <= k <= RDX_MMR_MAX_K, k <= fetch_k <= RDX_MMR_MAX_FETCH,
 * 0 <= lambda <= 1 (a NaN is refused). RDX_ERR_STATE on an index with mapped row ids (a shard). */
#define RDX_MMR_MAX_FETCH 1024
#define RDX_MMR_MAX_K 64
int rdx_index_mmr(rdx_index* h, const float* cand_score, const int64_t* cand_row, const int32_t* cand_count, int64_t nq, int fetch_k,
                  int k, double lambda, int32_t* out_pos, int64_t* out_row, float* out_score, double* out_value, int32_t* out_count,
                  int32_t* out_bad, void* stream);

/* Threshold search ------------------------------------------------------------------------------ */
/* Which allowed rows score at least t against a query, and how many: the question the reference asks on every request by fetching a
 * fixed 50 chunks and dropping those with distance > 0.30 on the host (src/rag/validators.py:64-81). rag_dpo_amd/range_search.py states
 * the definition and turns a distance into t; DESIGN.md §23.
 *
 * rdx_index_range. Per query q, with t = thresholds[q]: the ranking is rdx_search's (the same exact fp32 scores, score descending, row
 * ascending); a row is in range iff it is allowed and its score >= t (float comparison; t = -inf: every allowed row, t = +inf: none).
 *   out_total int64 [nq]: the rows in range, exact, whatever max_results.
 *   out_score fp32 / out_row int64 [nq][max_results]: the first min(max_results, total) entries of the ranking; padding -inf / -1.
 *   out_count int32 [nq]: min(max_results, total).
 *   out_paths HOST int32[2] (may be NULL): queries answered by the MFMA path (threshold from t, main scan, exact re-score of the hits) /
 *     by the exact full scan (small problems, option force_exact, and queries whose hits overflowed a segment or the hit list).
 * Both paths return the same bits. All other pointers are device pointers; the work is enqueued on `stream` and the call returns when the
 * results are complete. A pending asynchronous search is completed first. The search options force_exact, force_fast, force_bn,
 * small_scan, fuse_epilogue, cand_cap and refine_list steer it; the statistics and the feedback state of rdx_search are not touched.
 * RDX_ERR_INVALID before anything is enqueued: max_results outside [1, RDX_RANGE_MAX_RESULTS], nq outside [0, 65535], a mask made for
 * another device or row count. A NaN threshold or a query holding NaN/Inf: RDX_ERR_INVALID after the run,
 * the outputs undefined. RDX_ERR_STATE on an index with mapped row ids (a shard). */
#define RDX_RANGE_MAX_RESULTS 1024
int rdx_index_range(rdx_index* h, const float* queries, int64_t nq, const float* thresholds, int max_results, const rdx_mask* mask,
                    float* out_score, int64_t* out_row, int32_t* out_count, int64_t* out_total, int32_t* out_paths, void* stream);

/* Near-duplicate clustering ---------------------------------------------------------------------- */
/* Which stored rows are near-copies of which others: the threshold search asked of the corpus itself, and the answers joined into
 * connected components on the device. rag_dpo_amd/dedup.py states the definition; DESIGN.md §24.
 *
 * rdx_index_near_dup. "Allowed" = every row, or the rows of `mask`. For an allowed row i, R(i) = the allowed rows whose exact fp32
 * score against the stored row i (as a query: through the normalisation of every search) is >= threshold: what rdx_index_range
 * counts for that query. The graph has an edge i - j for every j in R(i), j != i, in either direction.
 *   out_label int64 [rows] (device): the smallest row of the row's connected component; -1 for a row that is not allowed.
 *   out_total int64 [rows] (device): |R(i)| (the row itself counts when it is in range); 0 for a row that is not allowed.
 *   out_stats HOST int64[4] (may be NULL): allowed rows examined / rows linked from their lists / rows linked by the dense pass /
 *     batches.
 * The allowed rows are taken as queries in batches (4 096; option "dup_batch"), gathered on the device: the rows never reach the
 * host. A row with at most list_cap rows in range is linked from the threshold search's list. A row with more ("heavy") is linked
 * from dense exact scores instead — none of a truncated list is used — at the cost of a quarter of an exact pass over the corpus;
 * when more than max_dense rows are heavy the call stops with RDX_ERR_INVALID (the distance is too loose for duplicate detection;
 * the message names the count and list_cap) and the outputs are undefined. Labels and totals do not depend on list_cap, the batch
 * size, the path or the schedule. The work is enqueued on `stream`; the call returns when the results are complete. A pending
 * asynchronous search is completed first; an empty index returns RDX_OK. The options that steer rdx_index_range steer it here; the
 * statistics and the feedback state of rdx_search are not touched.
 * RDX_ERR_INVALID before anything is enqueued: list_cap outside [1, RDX_RANGE_MAX_RESULTS], a NaN threshold, max_dense < 0, a mask
 * made for another device or row count, 2^31 rows or more. RDX_ERR_STATE on an index with mapped row ids (a shard). */
int rdx_index_near_dup(rdx_index* h, float threshold, const rdx_mask* mask, int list_cap, int64_t max_dense, int64_t* out_label,
                       int64_t* out_total, int64_t* out_stats, void* stream);

/* k-means of the stored rows ---------------------------------------------------------------------- */
/* Which themes the corpus holds and which rows belong to each: spherical k-means (Lloyd's iterations) over the stored rows, every
 * step in a stated order so that the answer is a function of the rows, `init`, max_iter and the mask alone.
 * rag_dpo_amd/kmeans.py states the definition; DESIGN.md §27.
 *
 * rdx_index_kmeans. "Allowed" = every row, or the rows of `mask`. score(c, r) = rdx_search's exact fp32 score of row r for the query c
 * (through the normalisation of every search). assign(C): every allowed row goes to the centroid with the largest score (compared as
 * fp32 values, ties to the smaller index). update: a cluster's members in ascending row order are cut into segments of 256; per
 * element a segment's total is the sequential fp64 sum of its members' stored values from +0.0, the cluster's sum the sequential fp64
 * sum of its segments' totals from +0.0; the new centroid is the normalisation (as of an added row) of the sums rounded to fp32; a
 * cluster without members keeps its centroid. C = normalised init; assign; then at most max_iter times update + assign, stopping
 * after the first assignment that changes no label (converged).
 *   init         fp32 [n_clusters][dim] (device; must not overlap out_centroid)
 *   out_label    int64 [rows] (device): the row's cluster under out_centroid; -1 for a row that is not allowed
 *   out_score    fp32 [rows] (device): its score against that centroid; -inf for a row that is not allowed
 *   out_centroid fp32 [n_clusters][dim] (device): the final centroids (max_iter = 0: the normalised init)
 *   out_count    int64 [n_clusters] (device): members per cluster
 *   out_info     HOST int32[2]: updates run, converged (0/1); written on success only
 * The work is enqueued on `stream`; the host reads one pinned word per assignment (the number of changed labels) and the call returns
 * when the results are complete. A pending asynchronous search is completed first; the statistics and the feedback state of
 * rdx_search are not touched. Labels, scores, centroids and counts do not depend on block sizes, the path or the schedule.
 * RDX_ERR_INVALID before anything is enqueued, the outputs untouched: n_clusters outside [1, RDX_KMEANS_MAX_CLUSTERS], max_iter outside
 * [0, RDX_KMEANS_MAX_ITER], a mask made for another device or row count, 2^31 rows or more, an empty index, a null or misaligned
 * pointer (init and out_centroid: 16 bytes). A NaN or Inf in init: RDX_ERR_INVALID after its normalisation ran, the outputs undefined.
 * RDX_ERR_STATE on an index with mapped row ids (a shard). */
#define RDX_KMEANS_MAX_CLUSTERS 4096
#define RDX_KMEANS_MAX_ITER 1000
int rdx_index_kmeans(rdx_index* h, const float* init, int n_clusters, int max_iter, const rdx_mask* mask, int64_t* out_label, float* out_score,
                     float* out_centroid, int64_t* out_count, int32_t* out_info, void* stream);

/* Value counts (facets) -------------------------------------------------------------------------- */
/* How many allowed rows carry each value of a metadata key: over the corpus, and over the rows within a distance of a query. The
 * reference asks the first with one full id list per value (src/processing/create_chromadb_index.py:447-480) and by counting fetched
 * metadata in a Python dict (pages/3_Documents.py:97-137). rag_dpo_amd/facets.py states the definitions; DESIGN.md §28.
 *
 * Both calls read a row -> code table: row_group int32 [rows of the index] (device), -1 = the row has no value, else a code in
 * [0, n_groups). Any other code raises a flag on the device and fails the call with RDX_ERR_INVALID after the run, the outputs
 * undefined; nothing is read or written through such a code. "Allowed" = every row, or the rows of `mask`.
 *
 * rdx_index_facet_count. out_counts int64 [n_groups] (device; may be NULL when n_groups == 0, and then row_group may be NULL too):
 * allowed rows per code. out_missing / out_total HOST int64[1]: allowed rows with code -1 / allowed rows (= the sum of out_counts +
 * missing). With n_groups == 0 the call counts the rows of a mask. The work is enqueued on `stream`; the call returns when the results
 * are complete. A pending asynchronous search is completed first; an empty index gives zeros.
 *
 * rdx_index_range_facets. Per query q, with t = thresholds[q]: the rows in range are rdx_index_range's — allowed, exact fp32 score >= t —
 * and they are counted by code instead of ranked.
 *   out_total   int64 [nq]: the rows in range (rdx_index_range's out_total, the same number).
 *   out_missing int64 [nq]: those of them with code -1.
 *   out_found   int32 [nq]: codes with a non-zero count (it may exceed limit).
 *   out_code int32 / out_n int64 [nq][limit]: the first min(limit, out_found) codes with a non-zero count by (count descending, code
 *     ascending) and their counts; padding -1 / 0.
 *   out_paths HOST int32[2] (may be NULL): as rdx_index_range's.
 * All other pointers are device pointers. Integers throughout: the results do not depend on the path, the batch, the option
 * "facet_table_kb" or the schedule. The queries are taken in passes whose uint32 tables [queries][n_groups] fit that option's budget
 * (default 262 144 = 256 MiB; 1..4194304; at least one query per pass whatever n_groups), at most 4 096 queries per pass. The options
 * that steer rdx_index_range steer it here; the statistics and the feedback state of rdx_search are not touched. The call returns when
 * the results are complete.
 * RDX_ERR_INVALID before anything is enqueued (both calls): n_groups outside [0, 2^31), limit outside [1, RDX_FACET_MAX_LIMIT], nq
 * outside [0, 65535], a null or misaligned pointer (queries: 16 bytes), a mask made for another device or row count, 2^31 rows or
 * more. A NaN threshold or a query holding NaN/Inf: RDX_ERR_INVALID after the run, the outputs undefined. RDX_ERR_STATE on an index
 * with mapped row ids (a shard). */
#define RDX_FACET_MAX_LIMIT 1024
int rdx_index_facet_count(rdx_index* h, const rdx_mask* mask, const int32_t* row_group, int64_t n_groups, int64_t* out_counts,
                          int64_t* out_missing, int64_t* out_total, void* stream);
int rdx_index_range_facets(rdx_index* h, const float* queries, int64_t nq, const float* thresholds, const rdx_mask* mask,
                           const int32_t* row_group, int64_t n_groups, int limit, int32_t* out_code, int64_t* out_n, int32_t* out_found,
                           int64_t* out_missing, int64_t* out_total, int32_t* out_paths, void* stream);

/* The combined BGE-M3 score ------------------------------------------------------------------------ */
/* score(question, chunk) = (w_dense dense + w_sparse sparse + w_colbert colbert) / (w_dense + w_sparse + w_colbert) over BGE-M3's three
 * outputs: rag_dpo_amd/m3.py states the definition once, in numpy, and drives the calls; DESIGN.md §31. The colbert component is
 * rdx_maxsim_f16's, the sparse one rdx_lex_score_pairs' (above), the dense one and the sum are the two calls here. Both take device
 * pointers only, are enqueued on `stream`, allocate and synchronise nothing, use no float atomics, and give an element the same bits
 * whatever its position, the call's length or its neighbours. Invalid scalars return RDX_ERR_INVALID before anything is launched.
 *
 * rdx_index_score_pairs. queries fp32 [nq][dim] are raw (16-byte aligned); each pair's query is normalised on the device exactly as
 * rdx_search normalises it. out_score[p] (fp32) is the exact score of rdx_search for query pair_q[p] (int32) and row pair_row[p]
 * (int64): the same summation order, the same bits, on the fp32 master and on a compact_master index alike. NaN, and nothing read
 * through the pair: a query outside [0, nq), a row outside [0, rows of the index), a query holding NaN or Inf. Limits: 1 <= nq <=
 * 65535, 1 <= n_pairs <= 2^20. RDX_ERR_STATE on an index with mapped row ids (a shard). One wave per pair (csrc/m3_kernel.hpp).
 *
 * rdx_m3_combine. value = ((w_dense * (double)dense + w_sparse * sparse) + w_colbert * (double)colbert) / W, W = (w_dense + w_sparse) +
 * w_colbert: three products, two sums and one division in fp64, each rounded once, never fused. A component whose weight is 0 is
 * skipped: it is not read and no 0 * x is added; its pointer must be NULL, and a component with a non-zero weight must not be
 * (RDX_ERR_INVALID otherwise). out_final fp32 [n] = (float)value; out_value f64 [n] (may be NULL) = value. A NaN component gives NaN.
 * Weights: finite, >= 0, W > 0 (a NaN is refused). 1 <= n <= 2^20. dense and colbert fp32 [n], sparse f64 [n]. */
int rdx_index_score_pairs(rdx_index* h, const float* queries, int64_t nq, const int32_t* pair_q, const int64_t* pair_row, int64_t n_pairs,
                          float* out_score, void* stream);
int rdx_m3_combine(int device, const float* dense, const double* sparse, const float* colbert, int64_t n, double w_dense, double w_sparse,
                   double w_colbert, float* out_final, double* out_value, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDX_H */
