/* The argument checks of rdx_meta_*, which come before the store handle is used and before any HIP call and so need no GPU: a
 * plain C program built with -fsanitize=address,undefined by tests/test_where_device.py. Every call must return RDX_ERR_INVALID
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
    if (sizeof(rdx_meta_leaf) != 24 || RDX_META_OP_NOT != RDX_DOCS_OP_NOT || RDX_META_OP_OR != RDX_DOCS_OP_OR) return 3;

    rdx_meta_leaf lv[17];
    for (int i = 0; i < 17; ++i) lv[i] = (rdx_meta_leaf){.col = 1, .op = RDX_META_EQ, .kind = 2, .code = -1, .num = 1.0};
    int32_t push17[17 + 16], deep[4098];
    for (int i = 0; i < 17; ++i) push17[i] = i;
    for (int i = 17; i < 33; ++i) push17[i] = RDX_META_OP_OR;
    for (int i = 0; i < 4098; ++i) deep[i] = (i & 1) ? RDX_META_OP_NOT : 0;
    const int32_t under[2] = {0, RDX_META_OP_AND}, not_first[1] = {RDX_META_OP_NOT}, two_left[2] = {0, 1}, one[1] = {0},
                  past[1] = {17}, unknown[1] = {-4};

    EXPECT_INVALID(rdx_meta_create(0, NULL), "null out");
    EXPECT_INVALID(rdx_meta_set_query(NULL, lv, 17, under, 2), "pops an empty stack");
    EXPECT_INVALID(rdx_meta_set_query(NULL, lv, 17, not_first, 1), "pops an empty stack");
    EXPECT_INVALID(rdx_meta_set_query(NULL, lv, 17, two_left, 2), "exactly one value");
    EXPECT_INVALID(rdx_meta_set_query(NULL, lv, 17, push17, 33), "more than 16 stack entries");
    EXPECT_INVALID(rdx_meta_set_query(NULL, lv, 16, push17, 31), "neither a leaf");        /* op 16 pushes leaf 16 of 16 */
    EXPECT_INVALID(rdx_meta_set_query(NULL, lv, 17, deep, 4098), "n_ops");
    EXPECT_INVALID(rdx_meta_set_query(NULL, lv, 17, deep, 0), "n_ops");
    EXPECT_INVALID(rdx_meta_set_query(NULL, lv, 17, NULL, 1), "n_ops");
    EXPECT_INVALID(rdx_meta_set_query(NULL, lv, 17, past, 1), "neither a leaf");
    EXPECT_INVALID(rdx_meta_set_query(NULL, lv, 17, unknown, 1), "neither a leaf");
    EXPECT_INVALID(rdx_meta_set_query(NULL, lv, 0, one, 1), "n_leaves");
    EXPECT_INVALID(rdx_meta_set_query(NULL, lv, RDX_META_MAX_LEAVES + 1, one, 1), "n_leaves");
    EXPECT_INVALID(rdx_meta_set_query(NULL, NULL, 1, one, 1), "n_leaves");
    rdx_meta_leaf bad = lv[0];
    bad.op = 7;
    EXPECT_INVALID(rdx_meta_set_query(NULL, &bad, 1, one, 1), "unknown op");
    bad.op = -1;
    EXPECT_INVALID(rdx_meta_set_query(NULL, &bad, 1, one, 1), "unknown op");
    bad = lv[0], bad.kind = 0;
    EXPECT_INVALID(rdx_meta_set_query(NULL, &bad, 1, one, 1), "kind");
    bad.kind = 5;
    EXPECT_INVALID(rdx_meta_set_query(NULL, &bad, 1, one, 1), "kind");
    bad = lv[0], bad.kind = 1, bad.op = RDX_META_LT;
    EXPECT_INVALID(rdx_meta_set_query(NULL, &bad, 1, one, 1), "EQ only");
    bad = lv[0], bad.col = -1;
    EXPECT_INVALID(rdx_meta_set_query(NULL, &bad, 1, one, 1), "out of range");
    bad.col = RDX_META_MAX_COLUMNS;
    EXPECT_INVALID(rdx_meta_set_query(NULL, &bad, 1, one, 1), "out of range");
    bad.op = RDX_META_CONST1;                                                               /* a CONST leaf's col is not read */
    EXPECT_INVALID(rdx_meta_set_query(NULL, &bad, 1, one, 1), "null store");
    EXPECT_INVALID(rdx_meta_set_query(NULL, lv, 17, push17 + 1, 31), "null store");         /* 16 entries: a legal query */

    const uint8_t kind[3] = {0, 4, 5};
    const double num[3] = {0, 1, 2};
    const int32_t code[3] = {-1, -1, -1};
    EXPECT_INVALID(rdx_meta_set_rows(NULL, 0, 0, kind, num, code, 3), "not one of 0 .. 4");
    EXPECT_INVALID(rdx_meta_set_rows(NULL, 0, 0, kind, num, code, 2), "null store");
    EXPECT_INVALID(rdx_meta_set_rows(NULL, -1, 0, kind, num, code, 2), "out of range");
    EXPECT_INVALID(rdx_meta_set_rows(NULL, RDX_META_MAX_COLUMNS, 0, kind, num, code, 2), "out of range");
    EXPECT_INVALID(rdx_meta_set_rows(NULL, 0, -1, kind, num, code, 2), "first_row");
    EXPECT_INVALID(rdx_meta_set_rows(NULL, 0, 0, kind, num, code, -1), "first_row");
    EXPECT_INVALID(rdx_meta_set_rows(NULL, 0, 2147483646, kind, num, code, 2), "first_row");
    EXPECT_INVALID(rdx_meta_set_rows(NULL, 0, 0, NULL, num, code, 2), "null kind");
    EXPECT_INVALID(rdx_meta_set_rows(NULL, 0, 0, kind, NULL, code, 2), "null kind");
    EXPECT_INVALID(rdx_meta_set_rows(NULL, 0, 0, kind, num, NULL, 2), "null kind");
    EXPECT_INVALID(rdx_meta_drop_column(NULL, -1), "out of range");
    EXPECT_INVALID(rdx_meta_drop_column(NULL, 0), "null store");
    EXPECT_INVALID(rdx_meta_truncate(NULL, -1), "rows < 0");
    EXPECT_INVALID(rdx_meta_truncate(NULL, 0), "null store");
    int64_t columns = 0, bytes = 0;
    uint32_t words[1] = {0};
    EXPECT_INVALID(rdx_meta_stats(NULL, &columns, &bytes), "null pointer");
    EXPECT_INVALID(rdx_meta_filter(NULL, 1, NULL, words, RDX_HOST, NULL), "null pointer");
    if (rdx_meta_destroy(NULL) != RDX_OK) return 4;
    printf("meta error paths ok: %d checks\n", n_checked);
    return 0;
}
