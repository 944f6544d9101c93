/* The argument checks of rdx_docs_*, which come before the store handle is used and before any HIP call and so need no GPU: a
 * plain C program built with -fsanitize=address,undefined by tests/test_where_document.py. Every call must return RDX_ERR_INVALID
 * with a message, read nothing past the (deliberately exact) arrays, and leave the process alive. The handle is NULL throughout:
 * a call that got past its argument checks answers "null store", which is RDX_ERR_INVALID too, so the order of the checks shows
 * in the message only — the cases below that must fail EARLIER say which word the message has to carry. */
#include <stdio.h>
#include <string.h>

#include "rdx.h"

#define EXPECT_INVALID(call, word)                                                                      \
    do {                                                                                                \
        int rc_ = (call);                                                                               \
        if (rc_ != RDX_ERR_INVALID || rdx_last_error() == NULL || strstr(rdx_last_error(), word) == NULL) { \
            fprintf(stderr, "%s -> %d (wanted %d with \"%s\"): %s\n", #call, rc_, RDX_ERR_INVALID, word, rdx_last_error()); \
            return 1;                                                                                   \
        }                                                                                               \
        ++n_checked;                                                                                    \
    } while (0)

int main(void) {
    int n_checked = 0;
    if (rdx_version() != RDX_ABI_VERSION) return 2;

    /* 17 patterns of one byte each */
    uint8_t pat[17];
    int64_t off[18], off_from1[18], off_empty[18];
    for (int i = 0; i < 17; ++i) pat[i] = (uint8_t)('a' + i);
    for (int i = 0; i < 18; ++i) off[i] = i, off_from1[i] = i + 1, off_empty[i] = i < 9 ? i : i - 1;   /* pattern 8 is empty */
    int32_t push17[17 + 16], deep[4097];
    for (int i = 0; i < 17; ++i) push17[i] = i;
    for (int i = 17; i < 33; ++i) push17[i] = RDX_DOCS_OP_OR;
    for (int i = 0; i < 4097; ++i) deep[i] = (i & 1) ? RDX_DOCS_OP_NOT : 0;
    const int32_t under[2] = {0, RDX_DOCS_OP_AND}, not_first[1] = {RDX_DOCS_OP_NOT}, two_left[2] = {0, 1}, one[1] = {0},
                  past[1] = {17}, unknown[1] = {-4};

    EXPECT_INVALID(rdx_docs_create(0, NULL), "null out");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, 0, one, 1), "P must be");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, RDX_DOCS_MAX_LEAVES + 1, one, 1), "P must be");
    EXPECT_INVALID(rdx_docs_set_query(NULL, NULL, off, 17, one, 1), "null pattern bytes");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, NULL, 17, one, 1), "null offsets");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off_from1, 17, one, 1), "offsets[0]");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off_empty, 17, one, 1), "strictly increasing");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, 17, deep, -1), "n_ops");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, 17, deep, 4097), "n_ops");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, 17, NULL, 1), "n_ops");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, 17, under, 2), "pops an empty stack");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, 17, not_first, 1), "pops an empty stack");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, 17, two_left, 2), "exactly one value");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, 17, push17, 33), "more than 16 stack entries");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, 17, past, 1), "neither a leaf");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, 16, push17, 31), "neither a leaf");   /* op 16 pushes leaf 16 of 16 */
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, 17, unknown, 1), "neither a leaf");
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, 17, push17 + 1, 31), "null store");   /* 16 entries: a legal query */
    EXPECT_INVALID(rdx_docs_set_query(NULL, pat, off, 17, NULL, 0), "null store");          /* leaves only: a legal query */

    /* three rows: "ab", "", "c" */
    const uint8_t text[3] = {'a', 'b', 'c'};
    const int64_t rows[4] = {0, 2, 2, 3}, rows_from1[4] = {1, 2, 2, 3}, rows_down[4] = {0, 2, 1, 3}, ids[3] = {0, 1, 2};
    EXPECT_INVALID(rdx_docs_append(NULL, text, rows, -1), "n < 0");
    EXPECT_INVALID(rdx_docs_append(NULL, text, NULL, 3), "null offsets");
    EXPECT_INVALID(rdx_docs_append(NULL, text, rows_from1, 3), "offsets[0]");
    EXPECT_INVALID(rdx_docs_append(NULL, text, rows_down, 3), "non-decreasing");
    EXPECT_INVALID(rdx_docs_append(NULL, NULL, rows, 3), "null bytes");
    EXPECT_INVALID(rdx_docs_append(NULL, text, rows, 3), "null store");
    EXPECT_INVALID(rdx_docs_replace(NULL, ids, text, rows, -1), "bad argument");
    EXPECT_INVALID(rdx_docs_replace(NULL, NULL, text, rows, 3), "bad argument");
    EXPECT_INVALID(rdx_docs_replace(NULL, ids, text, NULL, 3), "null offsets");
    EXPECT_INVALID(rdx_docs_replace(NULL, ids, text, rows_down, 3), "non-decreasing");
    EXPECT_INVALID(rdx_docs_replace(NULL, ids, NULL, rows, 3), "null bytes");
    EXPECT_INVALID(rdx_docs_replace(NULL, ids, text, rows, 3), "null store");
    EXPECT_INVALID(rdx_docs_compact(NULL, ids, 3), "rdx_docs_compact: bad argument");
    int64_t n_rows = 0, live = 0, arena = 0;
    uint32_t words[1] = {0};
    EXPECT_INVALID(rdx_docs_stats(NULL, &n_rows, &live, &arena), "rdx_docs_stats: null pointer");
    EXPECT_INVALID(rdx_docs_contains(NULL, words, RDX_HOST, NULL), "rdx_docs_contains: null pointer");
    EXPECT_INVALID(rdx_docs_filter(NULL, NULL, words, RDX_HOST, NULL), "rdx_docs_filter: null pointer");
    if (rdx_docs_destroy(NULL) != RDX_OK) return 4;
    printf("docs error paths ok: %d checks\n", n_checked);
    return 0;
}
